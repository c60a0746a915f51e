// mixture_plan.cpp -- the launch decision of the fused mixture kernel (sbayes_amd/csrc/sbe_mixture_plan.h) without a GPU:
// reads one case per line from stdin as key=value words and prints one JSON line per case (tests/test_mixture_plan_cpu.py).
//   creation:  N F S C Gtot slots cu  [ft= rows_ft=: the SBE_FT / SBE_ROWS_FT values]  [direct=1: SBE_DIRECT]
//   overrides of the derived shape (hand-made shapes):  o_direct o_partials
//   tuning:    kernel rows_sorted min_batch min_obs wide_min_share small_sl4 split shared in_kernel
//   launch:    n P KT share_ok epilogue waits
#include "../../sbayes_amd/csrc/sbe_mixture_plan.h"

#include <iostream>
#include <map>
#include <sstream>
#include <string>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::map<std::string, long long> kv;
        std::istringstream words(line);
        for (std::string w; words >> w;) {
            const size_t eq = w.find('=');
            if (eq == std::string::npos) { std::fprintf(stderr, "bad word: %s\n", w.c_str()); return 2; }
            kv[w.substr(0, eq)] = std::stoll(w.substr(eq + 1));
        }
        if (kv.empty()) continue;
        auto get = [&](const char* k, long long dflt) { auto it = kv.find(k); return it == kv.end() ? dflt : it->second; };
        sbe::MixShape s;
        int ft = (int)get("ft", 0), rows_ft = (int)get("rows_ft", 0);
        if (!sbe::derive_mix_shape(s, (int)get("N", 1), (int)get("F", 1), (int)get("S", 1), (int)get("C", 1), (int)get("Gtot", 1), (int)get("slots", 1),
                                   (int)get("cu", 256), kv.count("ft") ? &ft : nullptr, get("direct", 0) == 1, kv.count("rows_ft") ? &rows_ft : nullptr)) {
            std::printf("{\"shape_refused\": true}\n");
            continue;
        }
        if (kv.count("o_direct")) s.direct = get("o_direct", 0) != 0;
        if (kv.count("o_partials")) s.partials_stride = get("o_partials", 0);
        sbe::MixTuning t;
        t.opt_kernel = (int)get("kernel", t.opt_kernel);
        t.opt_rows_sorted = (int)get("rows_sorted", t.opt_rows_sorted);
        t.mfma_min_batch = (int)get("min_batch", t.mfma_min_batch);
        t.mfma_min_obs = get("min_obs", t.mfma_min_obs);
        t.mfma_wide_min_share = (int)get("wide_min_share", t.mfma_wide_min_share);
        t.mfma_small_sl4 = (int)get("small_sl4", t.mfma_small_sl4);
        t.mfma_split = (int)get("split", 0);
        t.shared_allowed = get("shared", 1) != 0;
        t.in_kernel_allowed = get("in_kernel", 1) != 0;
        sbe::MixFacts f;
        f.n = (int)get("n", 1); f.P = (int)get("P", 1); f.KT = (int)get("KT", 0);
        f.share_ok = get("share_ok", 0) != 0; f.epilogue = get("epilogue", 0) != 0; f.waits = get("waits", 0) != 0;
        const sbe::MixPlan p = sbe::plan_mixture(s, t, f);
        char name[128] = "";
        if (!p.err) sbe::plan_name(p, s, name, sizeof name);
        const int KT8 = f.KT >= 1 && f.KT <= 8;
        std::printf("{\"err\": %d, \"text\": \"%s\", \"form\": %d, \"grid\": %u, \"lds\": %zu, \"SL\": %d, \"MT\": %d, \"n_split\": %d, \"nt_per_split\": %d, "
                    "\"n_partials\": %d, \"in_kernel\": %d, \"done_blocks\": %u, \"ft\": %d, \"shape_ft\": %d, \"direct\": %d, \"rows_ft\": %d, \"state_h\": %d, "
                    "\"units4\": %lld, \"units16\": %lld}\n",
                    p.err, p.err ? p.msg : name, (int)p.form, p.grid_x, p.lds_bytes, p.SL, p.MT, p.n_split, p.nt_per_split, p.n_partials, (int)p.in_kernel,
                    p.done_blocks, p.ft, s.ft, (int)s.direct, s.rows_ft, (int)s.has_state_h,
                    KT8 ? (long long)sbe::tuple_mfma_units(s, f.n, 4, 1) : -1LL, KT8 ? (long long)sbe::tuple_mfma_units(s, f.n, 16, sbe::plan_div_up(f.KT, 2)) : -1LL);
    }
    return 0;
}
