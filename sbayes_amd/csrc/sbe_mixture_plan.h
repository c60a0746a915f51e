// sbe_mixture_plan.h -- which form of the fused mixture kernel a launch runs, and with what geometry: the whole decision of
// launch_mixture (sbe_engine_internal.hip.h) and the creation-time half of it (sbe_create), as plain C++17.  Host only, no HIP
// and nothing of the engine object: the engine hands over what creation fixed (MixShape), the option / experiment values
// (MixTuning; the header reads no environment variable) and what one launch contributes (MixFacts), and gets back a MixPlan --
// the form, its geometry, the grid, where the final reduction runs, or the refusal.  The pure numbers the decision shares with
// the kernels are defined here, once; the kernel headers include this file.  tests/c/mixture_plan.cpp drives it without a GPU
// (tests/test_mixture_plan_cpu.py): the thresholds below are pinned there.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/sbe_engine.h"      // SBE_MIXTURE_*, SBE_ERR_* (plain C)

namespace sbe {

// ---- numbers shared with the kernels --------------------------------------------------------------------------------------
constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kMaxComponents = 8;
constexpr int kMaxTuples = 64;
constexpr int kLogTabEntries = 128;               // intervals of tab_log_pos' table (sbe_device_common.hip.h)
constexpr int kRowsBlock = 1024;                  // k_mixture_rows
constexpr int kRowsWaves = kRowsBlock / kWave;
// waves per block of k_mixture_tuple64.  (8-wave blocks -- twice the waves per SIMD at the same LDS footprint -- were
// measured twice: 72.7 us at 80 VGPRs / 3 blocks per CU, 107 us at 64 VGPRs / 4 blocks per CU, against 61-63 us: the
// kernel does not fit those register budgets without spilling in its table build.)
constexpr int tuple64_waves() { return 4; }
constexpr int kTupleMfmaKBlockObjects = 64;       // objects per k-block of the FP4 count contraction (k_mixture_tuple_mfma)
constexpr int kTupleMfmaColsPerPass = 2;          // column tiles a wave of k_mixture_tuple_mfma owns per pass (= columns per lane)
constexpr int kMfmaWaves = 8;                     // waves per block of k_mixture_tuple_mfma
constexpr int kFineLogEntries = 1024;             // intervals of its own log table (tab_log4_n, sbe_mixture_mfma.hip.h)

constexpr size_t kLdsBytes = 160 * 1024;          // LDS of one CU: the most a block's dynamic image may take
constexpr size_t kRowsLdsMax = kLdsBytes - 512;   // ... of k_mixture_rows, which also has a few static words
constexpr size_t kLargeImage = 72 * 1024;         // from here on a staged image leaves room for ONE block per CU

inline int plan_div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
inline int plan_round_up(int a, int b) { return (a + b - 1) / b * b; }

// slots per block of the matrix-pipe form for KT tuples (0: the form does not apply): 16 up to 8 tuples, 4 up to 32, 2 up to 64
inline int tuple_mfma_slots_per_block(int KT) {
    if (KT < 1 || KT > 64) return 0;
    return KT <= 8 ? 16 : KT <= 32 ? 4 : 2;
}
// its LDS image: log table | A fragments | meta (32 MT entries whatever the form) | reduction
inline size_t tuple_mfma_lds_bytes(int MT, int C, int KBp) {
    const size_t meta = (size_t)32 * MT * (C <= 1 ? 8 : (C <= 3 ? 16 : 32));
    return (size_t)MT * KBp * 1024 + kFineLogEntries * 16 + meta + (size_t)kMfmaWaves * 2 * 16 * sizeof(double);
}

// ---- what creation fixes ---------------------------------------------------------------------------------------------------
struct MixShape {
    int N = 0, F = 0, S = 0, C = 0, n_slots = 0;
    int Gtot = 0, Pmax = 0;
    int Np = 0, NQ = 0;            // objects padded to a multiple of 4; object quads
    int Fq = 0;                    // padded features: row pitch of the quad-interleaved state streams (>= any tiling of F)
    int ft = 64, n_ftiles = 0;     // v2 fused-kernel feature tile width, tiles
    bool direct = false;           // tables of a 16-feature tile exceed LDS: gather from the global tiled tables
    int rows_ft = 0;               // tile width of k_mixture_rows (32 / 16; 0: its LDS image does not fit, or C > 4)
    bool has_state_h = false;      // the prepared LDS-offset stream of k_mixture_tuple64 exists (ft == 64, S <= 127)
    int compute_units = 256;
    int64_t partials_stride = 0;   // partial sums per slot the engine has room for

    int64_t table_elems() const { return (int64_t)Gtot * F * S; }
    int64_t tile_tab_elems() const { return (int64_t)(Gtot + 1) * S * ft; }
};

// The shape of an engine of n_objects x n_features x n_states with n_components components of gtot groups in all.  forced_ft /
// forced_rows_ft: the values of SBE_FT / SBE_ROWS_FT, or null where the variable is not set; force_direct: SBE_DIRECT=1.
// false: the forced tile width's tables do not fit LDS (nothing else can fail).
inline bool derive_mix_shape(MixShape& s, int n_objects, int n_features, int n_states, int n_components, int gtot, int n_slots,
                             int compute_units, const int* forced_ft, bool force_direct, const int* forced_rows_ft) {
    s = MixShape{};
    s.N = n_objects; s.F = n_features; s.S = n_states; s.C = n_components; s.n_slots = n_slots;
    s.Gtot = gtot;
    s.Pmax = std::min(1 << n_components, 64);
    s.Np = plan_round_up(n_objects, 4);
    s.NQ = s.Np / 4;
    s.compute_units = compute_units;
    {   // v2 feature-tile width: widest of 64/32/16 whose LDS image leaves two blocks per CU
        int ft = 64;
        auto lds_for = [&](int t) { return ((size_t)(gtot + 1) * t * n_states) * sizeof(float) + (size_t)s.Pmax * n_components * t * sizeof(double) + 8 * 1024; };
        while (ft > 16 && lds_for(ft) > 78 * 1024) ft >>= 1;
        if (forced_ft && (*forced_ft == 64 || *forced_ft == 32 || *forced_ft == 16)) ft = *forced_ft;
        if (lds_for(ft) > 156 * 1024) {
            if (forced_ft) return false;
            ft = 16;                 // very many groups x states: no LDS staging of tables (L2-served gathers)
            s.direct = true;
        }
        if (force_direct) { ft = 16; s.direct = true; }   // experiments / tests
        s.ft = ft;
        s.n_ftiles = plan_div_up(n_features, ft);
        s.Fq = plan_round_up(n_features, 64);
    }
    if (n_components <= 4) {   // k_mixture_rows: widest tile whose LDS image (tables f32 [(Gtot+1)][S+1][ft] + f64 weight planes) fits
        // (sized for half the possible has_components patterns: a component every object has -- `universal` -- halves
        //  them; a launch whose slots really have more falls back to k_mixture_v2) + the waves' offset slots
        const int64_t S = n_states, C = n_components;
        const int p_assumed = std::max(1, s.Pmax / 2);
        auto rows_lds = [&](int t) { return (size_t)(gtot + 1) * (S + 1) * t * 4 + (size_t)p_assumed * ((C + 1) / 2) * t * 16 + (size_t)kRowsWaves * (kWave / t) * (C + 1) * 16; };
        s.rows_ft = rows_lds(32) <= kRowsLdsMax ? 32 : rows_lds(16) <= kRowsLdsMax ? 16 : 0;
        if (forced_rows_ft) { const int v = *forced_rows_ft; if (v == 0 || ((v == 16 || v == 32) && rows_lds(v) <= kRowsLdsMax)) s.rows_ft = v; }
    }
    s.has_state_h = s.ft == 64 && n_states <= 127 && (int64_t)s.NQ * s.Fq * 8 < ((int64_t)1 << 31);
    {   // partials: worst-case block count of the fused kernel (ft = 16, one packed step per thread)
        const int64_t min_objs = kBlock / (16 / 4);
        s.partials_stride = std::max<int64_t>(plan_div_up(n_features, 16) * std::max<int64_t>(plan_div_up(n_objects, min_objs), 4 * compute_units), 1024);
    }
    return true;
}

// ---- options and experiment values (the engine reads the environment; see sbe_create and launch_mixture) ------------------
struct MixTuning {
    int opt_kernel = SBE_MIXTURE_PACKED;
    int opt_rows_sorted = 1;         // SBE_ROWS_SORTED: 0 never, 1 launches of >= 16 slots at 32-feature tiles (default), 2 whenever it applies (tests)
    int mfma_min_batch = 320;        // smallest launch the matrix-pipe form is chosen for under SBE_MIXTURE_PACKED (SBE_MFMA_MIN_BATCH);
                                     // round 6, FP4 operands: 24.5 / 24.6 / 24.8 us against 22.2 / 32.1 / 34.9 us of k_mixture_tuple64 at
                                     // 256 / 384 / 512 headline states (tools/diag/mfma_threshold.py, profiles/r6/mfma_threshold.log)
    int64_t mfma_min_obs = 6400000;  // ... chosen from 32 states per launch on when n x N x F reaches this (SBE_MFMA_MIN_OBS)
    int mfma_wide_min_share = 16;    // wide matrix-pipe forms (> 8 tuples) by default only from this many objects per padded tuple on (SBE_MFMA_WIDE_MIN_SHARE)
    int mfma_small_sl4 = 1;          // four slots per block for launches whose blocks fit two rounds on the CUs (SBE_MFMA_SMALL_SL4=0: A/B)
    int mfma_split = 0;              // SBE_MFMA_SPLIT (> 0: that many column splits; experiments), read at every launch that considers the matrix pipe
    bool shared_allowed = true;      // the shared-operand epilogue where it applies (SBE_MFMA_SHARED=0: never); fixed for the process
    bool in_kernel_allowed = true;   // the kernel finishes the reduction itself where it pays (SBE_REDUCE_IN_KERNEL=0: never); fixed for the process
};

// ---- what one launch contributes -------------------------------------------------------------------------------------------
struct MixFacts {
    int n = 1;                 // slots of the launch
    int P = 1;                 // most has_components patterns of any of its slots (>= 1)
    int KT = 0;                // most group tuples of any of its slots; 0: some slot has no tuple table
    bool share_ok = false;     // every slot's tuple tables fit the shared-operand epilogue
    bool epilogue = false;     // a step epilogue rides on the reduction (fin / d_fins)
    bool waits = false;        // the caller waits on a completion flag (done_out)
};

enum class MixForm : int { TupleMfma, Tuple64, Combo, Rows, RowsSorted, OnehotV2, V2 };

struct MixPlan {
    int err = SBE_OK;          // SBE_ERR_*: the launch is refused, `msg` says why
    char msg[256] = {0};
    MixForm form = MixForm::V2;
    int P = 1, KT = 0;
    // every form but the matrix pipe: feature tiles x chunks of object quads
    int ft = 0, n_ftiles = 0, quads_per_chunk = 0, n_chunks = 0;
    bool onehot = false;       // the one-hot stream (combo / one-hot v2)
    size_t lds_bytes = 0;      // the block's dynamic LDS, whatever the form
    int combo_w_off = 0, combo_tab_off = 0;      // group-tuple forms on the vector pipe: byte offsets of the weight tile / the byte table
    int rs_nq_max = 0;         // pattern-sorted rows: the longest padded order a slot can have, in quads
    // matrix pipe: SL slots per block (16 / 4 / 2), MT M tiles, n_split column splits of nt_per_split column tiles
    int SL = 0, MT = 0, n_split = 0, nt_per_split = 0;
    bool shared = false;
    // XCD-aware 1-D grid (see k_mixture_v2): units = work items x slot groups, unit u on XCD u % 8
    int slot_groups = 1, slots_per_group = 1, gen_slots = 0, ragged_w = 0;
    unsigned grid_x = 0;
    int n_partials = 0;        // partial sums per slot
    bool in_kernel = false;    // the kernel's last block adds them; else k_reduce_partials
    unsigned done_blocks = 0;  // in_kernel: blocks that signal a waiting caller's completion flag
};

// cost of a matrix-pipe launch of n slots at SL slots per block and MT M tiles: rounds of blocks x passes per block x M tiles
inline int64_t tuple_mfma_units(const MixShape& s, int n, int SL, int MT) {
    const int NT = plan_div_up((int64_t)s.F * s.S, 32);
    const int groups = plan_div_up(n, SL);
    const int split = std::max(1, std::min(plan_div_up(NT, 16), s.compute_units / std::max(1, groups)));
    const int passes = plan_div_up(plan_round_up(plan_div_up(NT, split), 2), 16);
    return (int64_t)plan_div_up(groups * split, s.compute_units) * passes * MT;
}

// Whether a launch is considered for the matrix pipe at all (the engine reads SBE_MFMA_SPLIT for these launches only): forced, or
// by default from mfma_min_batch states per launch on whatever the shape, and -- four slots per block -- from 32 states on when
// the launch holds enough observations for the kernel's fixed costs: 32 headline states = 6.4 M
inline bool considers_tuple_mfma(const MixShape& s, const MixTuning& t, const MixFacts& f) {
    if (f.KT == 0) return false;
    if (t.opt_kernel == SBE_MIXTURE_PACKED_TUPLE_MFMA) return true;
    return t.opt_kernel == SBE_MIXTURE_PACKED &&
           (f.n >= t.mfma_min_batch || (t.mfma_small_sl4 && f.n >= 32 && (int64_t)f.n * s.N * s.F >= t.mfma_min_obs));
}

namespace plan_detail {

struct TileGeom { int ft, n_ftiles, quads_per_chunk, n_chunks, n_blocks; size_t lds_bytes; };

// v2 geometry: chunks of object quads; one wave step = 64/ft quads.  The chunk's ids are staged
// in LDS (8*C + 4 bytes per quad), which caps the chunk length.
inline TileGeom tile_geometry_v2(const MixShape& s, int P, int n_batch, int blocks_per_cu) {
    TileGeom g{};
    g.ft = s.ft;
    g.n_ftiles = s.n_ftiles;
    const size_t image = (size_t)s.tile_tab_elems() * sizeof(float) + (size_t)P * s.C * s.ft * sizeof(double);
    // no more workgroups than the CUs hold at once when the tile image is large: every workgroup stages the whole
    // image, so extra generations only multiply the staging traffic (stress shape, single eval: 15.9 -> 13 us)
    if (!s.direct) blocks_per_cu = (int)std::max<size_t>(1, std::min<size_t>((size_t)blocks_per_cu, kLdsBytes / (image + 4096)));
    const int64_t target_blocks = (int64_t)blocks_per_cu * s.compute_units;
    const int64_t chunks = std::max<int64_t>(1, target_blocks / ((int64_t)g.n_ftiles * std::max(1, n_batch)));
    const int min_quads = 4 * (kWave / s.ft);            // one step for each of the 4 waves
    const int max_quads = std::max(min_quads, (8 * 1024) / (8 * s.C + 4));
    g.quads_per_chunk = std::min<int>(max_quads, std::max<int>(min_quads, plan_div_up(s.NQ, chunks)));
    g.n_chunks = plan_div_up(s.NQ, g.quads_per_chunk);
    g.n_blocks = g.n_chunks * g.n_ftiles;
    g.lds_bytes = (size_t)g.quads_per_chunk * (8 * s.C + 4);
    if (!s.direct) g.lds_bytes += image;
    return g;
}

// geometry of a matrix-pipe launch over n slots with at most KT tuples each; n_split = 0: the form does not apply
struct MfmaGeom { int n_split, nt_per_split, MT, SL; size_t lds; };
inline MfmaGeom mfma_geometry(const MixShape& s, const MixTuning& t, int n, int KT) {
    MfmaGeom g{};
    g.SL = tuple_mfma_slots_per_block(KT);           // 16 slots x <= 8 tuples, 4 x <= 32, 2 x <= 64 per block: the most KT allows
    if (g.SL == 0 || s.C > 4) return g;
    const int NT = plan_div_up((int64_t)s.F * s.S, 32), KBp = plan_round_up(plan_div_up(s.N, kTupleMfmaKBlockObjects), 4);
    // Few states per launch: with 16 slots per block a launch of n states is ceil(n / 16) x (at most 4 column splits) blocks -- at
    // 512 states half the CUs idle and every block still walks a whole pass of MT M tiles (24.6 us at 256..1024 headline states).
    // Four slots per block (ONE M tile of <= 8 tuples x 4 slots) make four times the blocks of a third of the work per pass.  The
    // two geometries are compared by rounds of blocks x passes per block x M tiles (a pass costs ~4.3 us per M tile at the headline
    // shape): 14.6 / 16.1 / 17.9 / 21.4 us at 32 / 256 / 320 / 512 states (1 / 1 / 2 / 2 units against 3) where k_mixture_tuple64
    // takes 16.0 / 21.1 / 26.5 / 35.1 us; at 576 states the four-slot form needs 4 units (30.6 us) and the 16-slot form stays
    // (24.6 us): profiles/r6/mfma_threshold.log
    // (tuple_mfma_units)
    if (g.SL == 16 && t.mfma_small_sl4 && tuple_mfma_units(s, n, 4, 1) < tuple_mfma_units(s, n, 16, plan_div_up(KT, 2))) g.SL = 4;
    // ... and fewer slots per block while the A image -- MT x KBp KB, MT = tuples x slots / 32 -- does not fit a
    // CU's LDS: many objects with few tuples (5000 objects x 6 tuples: 16 slots need 3 x 80 KB, 4 slots 1 x 80 KB)
    for (;;) {
        g.MT = plan_div_up(KT, 32 / g.SL);
        g.lds = tuple_mfma_lds_bytes(g.MT, s.C, KBp);
        if (g.lds <= kLdsBytes || g.SL == 2) break;
        g.SL = g.SL == 16 ? 4 : 2;
    }
    if (g.lds > kLdsBytes) return g;
    // the tables are addressed through 32-bit buffer offsets
    const int64_t probs_bytes = ((int64_t)s.n_slots * s.table_elems() + (int64_t)s.F * s.S) * 4;
    const int64_t wpat_bytes = ((int64_t)s.n_slots * s.Pmax * s.F * s.C + (int64_t)s.F * s.C) * 4;
    if (probs_bytes >= ((int64_t)1 << 32) || wpat_bytes >= ((int64_t)1 << 32) || ((int64_t)(NT + 1) * KBp + 4) * 1024 >= ((int64_t)1 << 31)) return g;
    // one block = SL slots x a range of column tiles; its 8 waves take the tiles in pairs, so a split of fewer than
    // 16 tiles leaves waves idle: as many splits as fill the CUs, no finer
    const int groups = plan_div_up(n, g.SL);
    int n_split = std::max(1, std::min(plan_div_up(NT, 16), s.compute_units / std::max(1, groups)));
    if (t.mfma_split > 0) n_split = std::min(t.mfma_split, NT);   // experiments
    g.nt_per_split = plan_round_up(plan_div_up(NT, n_split), 2);
    // (the kernel sums count * binary exponent in 32-bit integers, one accumulator per lane and slot: in a pass of 16 tiles a
    //  lane adds the entries of its kTupleMfmaColsPerPass columns -- over every M tile and both tuples of a tile -- into the
    //  same accumulator, and a slot's counts of ONE column add up to at most N over its tuples; the exponents are summed
    //  BIASED (0 .. 2046; the bias leaves as 1023 x the columns' object count at the end), 2100 covers every double)
    if ((int64_t)plan_div_up(g.nt_per_split, 16) * kTupleMfmaColsPerPass * s.N * 2100 >= ((int64_t)1 << 31)) return g;
    g.n_split = plan_div_up(NT, g.nt_per_split);
    return g;
}

template <class... A>
inline MixPlan& refuse(MixPlan& p, int code, const char* fmt, A... a) {
    p.err = code;
    snprintf(p.msg, sizeof p.msg, fmt, a...);
    return p;
}

// ---- the decision, form by form (plan_mixture below puts them in order) -----------------------------------------------------
// Matrix pipe: large batches, the per-observation gather as an integer contraction (k_mixture_tuple_mfma).  false: not this form.
inline bool plan_tuple_mfma(MixPlan& p, const MixShape& s, const MixTuning& t, const MixFacts& f, size_t* lds_tried) {
    const int n = f.n, KT = f.KT;
    const bool forced = t.opt_kernel == SBE_MIXTURE_PACKED_TUPLE_MFMA;
    if (!considers_tuple_mfma(s, t, f)) return false;
    const MfmaGeom mg = mfma_geometry(s, t, n, KT);
    *lds_tried = mg.lds;
    if (mg.n_split == 0) return false;
    // The wide forms (more than 8 tuples: 4 / 2 slots per block) pay one log per (padded tuple, feature, state) where the
    // vector-pipe form pays one gather per observation: by default only where a table entry is shared by enough objects
    // (SBE_MFMA_WIDE_MIN_SHARE, objects per padded tuple; measured crossover: profiles/r6/wide_forms.log)
    if (!forced && KT > 8 && s.N < t.mfma_wide_min_share * mg.MT * (32 / mg.SL)) return false;
    p.form = MixForm::TupleMfma;
    p.SL = mg.SL; p.MT = mg.MT; p.n_split = mg.n_split; p.nt_per_split = mg.nt_per_split; p.lds_bytes = mg.lds;
    // the shared-operand epilogue: C = 2, 16 slots per block, at most 3 M tiles (6 tuples; 4 tiles spill), every slot of the
    // launch fitting it (per-slot flag)
    p.shared = s.C == 2 && mg.SL == 16 && mg.MT <= 3 && t.shared_allowed && f.share_ok;
    p.n_partials = mg.n_split;                   // one per column split
    p.grid_x = (unsigned)(plan_div_up(n, mg.SL) * mg.n_split);
    return true;
}

// Group-tuple form on the vector pipe: eligible when every slot of the launch has few distinct tuples, the log table fits
// LDS and a block sees enough observations to amortise building it.  It prefers long chunks (one block per CU is enough:
// the table build is per block), so it gets its own geometry.  false: not this form (*lds_tried: the image it would need).
inline bool plan_combo(MixPlan& p, TileGeom& g, const MixShape& s, const MixTuning& t, const MixFacts& f, size_t* lds_tried) {
    const int P = f.P, KT = f.KT;
    const bool forced = t.opt_kernel == SBE_MIXTURE_PACKED_TUPLE || t.opt_kernel == SBE_MIXTURE_PACKED_TUPLE_LDS;
    if (KT == 0 || !(forced || t.opt_kernel == SBE_MIXTURE_PACKED || t.opt_kernel == SBE_MIXTURE_ONEHOT)) return false;
    const TileGeom gc = tile_geometry_v2(s, P, f.n, 2);
    // 64-feature tiles, packed stream: the scalar-unit form (tuple metadata in VGPRs, no id staging)
    const bool tuple64 = !p.onehot && gc.ft == 64 && s.has_state_h && t.opt_kernel != SBE_MIXTURE_PACKED_TUPLE_LDS;
    // LDS image: T[KT][S+1][ft] f64 | tq[quads] u32 | tuple rows u16 | tuple patterns u32 | weights f64 [| byte table]
    //   (tuple64: T | weights)
    const int cu = s.C <= 4 ? s.C : kMaxComponents;
    size_t lds = (size_t)KT * (s.S + 1) * gc.ft * sizeof(double);
    if (!tuple64) {
        lds += (size_t)gc.quads_per_chunk * 4;
        lds += ((size_t)KT * cu + ((KT * cu) & 1)) * sizeof(uint16_t) + (size_t)KT * sizeof(uint32_t);
    }
    lds = (lds + 15) / 16 * 16;
    const int w_off = (int)lds;
    lds += (size_t)P * s.C * gc.ft * sizeof(double);
    if (tuple64) lds += tuple64_waves() * sizeof(double) + kLogTabEntries * 2 * sizeof(double);   // reduction scratch (the kernel has no static LDS) + log table
    const int tab_off = (int)lds;
    bool fits = true;
    if (p.onehot) {      // byte-position lookup table [seg16][32] u16; a tile row segment must fit one step
        const int seg16 = gc.ft * s.S / 16;
        fits = seg16 <= kBlock;
        lds += (size_t)seg16 * 32 * sizeof(uint16_t);
    }
    *lds_tried = lds;
    const int64_t obs_per_block = (int64_t)gc.quads_per_chunk * 4 * gc.ft;
    if (!fits || (forced ? lds > 150 * 1024 : (lds > 40 * 1024 || obs_per_block < (int64_t)3 * KT * s.S * gc.ft))) return false;
    g = gc;
    g.lds_bytes = lds;
    p.form = tuple64 ? MixForm::Tuple64 : MixForm::Combo;
    p.combo_w_off = w_off;
    p.combo_tab_off = p.onehot ? tab_off : 0;
    return true;
}

// Rows form (k_mixture_rows): the general packed kernel whenever its LDS image fits -- 1024-thread blocks over 32-feature (or
// 16-feature) tiles; SBE_MIXTURE_PACKED_V2 keeps the older k_mixture_v2 (A/B, tests).  false: not this form.
inline bool plan_rows(MixPlan& p, TileGeom& g, const MixShape& s, const MixTuning& t, const MixFacts& f) {
    const int n = f.n, rft = s.rows_ft;
    if (p.onehot || rft == 0 || t.opt_kernel == SBE_MIXTURE_PACKED_V2) return false;
    const size_t wave_slots = (size_t)kRowsWaves * (kWave / rft) * (s.C + 1) * 16;
    const size_t rows_image = (size_t)(s.Gtot + 1) * (s.S + 1) * rft * 4 + (size_t)f.P * ((s.C + 1) / 2) * rft * 16 + wave_slots;   // tables | weights | offset slots
    if (rows_image > kRowsLdsMax) return false;      // more patterns than the tile width was sized for
    if (t.opt_kernel != SBE_MIXTURE_PACKED_GENERAL) {
        // a single eval with a large image (stress shape: 153 KB per block) is staging-bound in the rows form (measured
        // 13.8 us against 12.5 us for k_mixture_v2's many small blocks); from two evals per launch on the rows form wins
        if (n == 1 && rows_image > kLargeImage) return false;
        // The rows form needs long object ranges (a 1024-thread block covers 32 quads per step) and enough observations
        // per launch to fill one block per CU; below that k_mixture_v2's 256-thread blocks win.  Thresholds from
        // tools/rows_crossover.py on an MI355X (kernel time of both forms over N = 500..5000, B = 8..256, C = 2 / 4,
        // and the stress shape itself): they depend on the tile width k_mixture_v2 would run at (64: efficient, 16: not).
        const int64_t obs = (int64_t)n * s.N * s.F;
        const int64_t min_obs = s.ft >= 64 ? 64000000 : s.ft >= 32 ? 24000000 : 10000000;
        const int min_quads = s.ft >= 64 ? 500 : s.ft >= 32 ? 375 : 250;
        if (obs < min_obs || s.NQ < min_quads) return false;
    }
    // pattern-sorted objects (weights in registers): 32-feature tiles, a second offsets slot per wave in LDS, state-row
    // offsets of 24 bits
    const size_t sorted_image = rows_image + wave_slots;
    const bool sorted = (t.opt_rows_sorted == 2 || (t.opt_rows_sorted == 1 && n >= 16)) && rft == 32 && sorted_image <= kRowsLdsMax &&
                        (int64_t)(s.N + 1) * s.Fq < ((int64_t)1 << 24) && s.Pmax <= 64;
    const int gran = kRowsWaves * (kWave / rft);         // quads per block step
    const int n_t = plan_div_up(s.F, rft);
    const size_t image = sorted ? sorted_image : rows_image;
    const int step_objs = 4 * (kWave / rft);
    p.rs_nq_max = plan_round_up(s.N + s.Pmax * (step_objs - 1), step_objs) / 4;
    const int NQ_geo = sorted ? p.rs_nq_max : s.NQ;      // (sorted: the longest padded order a slot can have)
    // every block stages the whole image: with a large image one block per CU and as few object chunks as fill
    // the chip; small images take two generations of blocks
    // (a block that stages a large image wants at least ~8 block steps of work behind it)
    const int64_t target = (int64_t)s.compute_units * (image > kLargeImage ? 1 : 2);
    const int min_steps = image > kLargeImage ? 8 : image > 24 * 1024 ? 4 : 1;
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(plan_div_up(NQ_geo, (int64_t)gran * min_steps), plan_div_up(target, (int64_t)n_t * n)));
    const int qpc = plan_round_up(plan_div_up(NQ_geo, chunks), gran);
    g.ft = rft; g.n_ftiles = n_t; g.quads_per_chunk = qpc; g.n_chunks = plan_div_up(NQ_geo, qpc);
    g.n_blocks = g.n_chunks * n_t; g.lds_bytes = image;
    p.form = sorted ? MixForm::RowsSorted : MixForm::Rows;
    return true;
}

// the grid of every form but the matrix pipe: XCD-aware and 1-D (see k_mixture_v2) -- units = work items x slot groups, unit u on XCD u % 8
inline void plan_tile_grid(MixPlan& p, const TileGeom& g, const MixShape& s, int n) {
    p.ft = g.ft; p.n_ftiles = g.n_ftiles; p.quads_per_chunk = g.quads_per_chunk; p.n_chunks = g.n_chunks;
    p.lds_bytes = g.lds_bytes;
    p.n_partials = g.n_blocks;
    int gcd8 = 8;
    while (g.n_blocks % gcd8) gcd8 >>= 1;
    p.slot_groups = std::max(1, std::min(8 / gcd8, n));
    p.slots_per_group = plan_div_up(n, p.slot_groups);
    p.grid_x = (unsigned)(8 * plan_div_up(g.n_blocks * p.slot_groups, 8) * p.slots_per_group);
    if (p.form != MixForm::Tuple64) return;
    // k_mixture_tuple64: own block order (slots dealt to XCDs, generations, heavy work items first; see the kernel)
    p.gen_slots = std::max(1, (4 * s.compute_units / 8) / g.n_blocks);
    const int gens = plan_div_up(plan_div_up(n, 8), p.gen_slots);
    p.grid_x = n >= 8 ? (unsigned)(8 * gens * p.gen_slots * g.n_blocks) : (unsigned)(n * g.n_blocks);
    p.ragged_w = (s.F % 64 != 0 && s.F % 64 <= 32) ? s.F % 64 : 0;
}

}  // namespace plan_detail

inline MixPlan plan_mixture(const MixShape& s, const MixTuning& t, const MixFacts& f) {
    using namespace plan_detail;
    MixPlan p{};
    p.P = f.P; p.KT = f.KT;
    p.onehot = t.opt_kernel == SBE_MIXTURE_ONEHOT || t.opt_kernel == SBE_MIXTURE_ONEHOT_GENERAL;
    size_t lds_tried = 0;
    const bool mfma = plan_tuple_mfma(p, s, t, f, &lds_tried);
    if (!mfma && t.opt_kernel == SBE_MIXTURE_PACKED_TUPLE_MFMA)
        return refuse(p, SBE_ERR_ARG, "matrix-pipe group-tuple kernel forced but not applicable (tuples=%d, C=%d, LDS %zu bytes)", f.KT, s.C, lds_tried);
    if (!mfma) {
        TileGeom g = tile_geometry_v2(s, f.P, f.n, 4);
        const bool combo = plan_combo(p, g, s, t, f, &lds_tried);
        if (!combo && (t.opt_kernel == SBE_MIXTURE_PACKED_TUPLE || t.opt_kernel == SBE_MIXTURE_PACKED_TUPLE_LDS))
            return refuse(p, SBE_ERR_ARG, "group-tuple kernel forced but not applicable (tuples=%d, LDS %zu bytes)", f.KT, lds_tried);
        if (!combo && !plan_rows(p, g, s, t, f)) p.form = p.onehot ? MixForm::OnehotV2 : MixForm::V2;
        plan_tile_grid(p, g, s, f.n);
    }
    if (p.n_partials > s.partials_stride)
        return refuse(p, SBE_ERR_STATE, "internal: partials buffer too small (%d > %lld)", p.n_partials, (long long)s.partials_stride);
    if ((p.form == MixForm::OnehotV2 || p.form == MixForm::V2) && p.lds_bytes > 159 * 1024)
        return refuse(p, SBE_ERR_ARG, "probability / weight tables too large for LDS staging at tile width %d (%zu bytes; G_total=%d, S=%d, P=%d)",
                      p.ft, p.lds_bytes, s.Gtot, s.S, f.P);
    // Without a step epilogue the kernel finishes the reduction itself (the last block of a slot -- of a group of 16 slots in
    // the matrix-pipe form -- adds the partial sums): one launch per eval (batch) instead of two.  SBE_REDUCE_IN_KERNEL=0
    // keeps k_reduce_partials (A/B runs).
    // Where it pays (measured, tools/probe/single_eval_latency.py and bench.py): always in the matrix-pipe form (two to four
    // blocks per 16 slots) and when a slot is ONE block (no tickets at all); for a few blocks per slot in the asynchronous
    // calls (throughput: one launch less per eval, cfg1 138 -> 164 k evals/s).  A host-synchronous call waits for the last
    // block's store -> ticket -> loads, three dependent trips to the coherence point, which is 1.2-2 us MORE than the second
    // launch; and with hundreds of blocks per slot the tickets at one address serialise (headline, one eval: 8.1 -> 11.2 us).
    p.in_kernel = !f.epilogue && t.in_kernel_allowed && (mfma || p.n_partials == 1 || (!f.waits && p.n_partials <= 16));
    if (p.in_kernel) p.done_blocks = (unsigned)(mfma ? plan_div_up(f.n, p.SL) : f.n);
    return p;
}

// the sbe_last_mixture_kernel string of a planned launch
inline void plan_name(const MixPlan& p, const MixShape& s, char* out, size_t cap) {
    if (p.form == MixForm::TupleMfma) {
        snprintf(out, cap, "k_mixture_tuple_mfma<packed stream, group-tuple form, matrix pipe fp4, %d slots x M tiles %d, C=%d%s>", p.SL, p.MT, s.C,
                 p.shared ? ", shared operands" : "");
        return;
    }
    const bool combo = p.form == MixForm::Tuple64 || p.form == MixForm::Combo;
    const char* kernel = p.form == MixForm::Tuple64 ? "k_mixture_tuple64" : p.form == MixForm::Combo ? "k_mixture_combo"
                       : (p.form == MixForm::Rows || p.form == MixForm::RowsSorted) ? "k_mixture_rows"
                       : p.form == MixForm::OnehotV2 ? "k_mixture_onehot_v2" : "k_mixture_v2";
    snprintf(out, cap, "%s<%s%s, tile %d, C=%d>", kernel, p.onehot ? "one-hot stream" : "packed stream",
             combo ? ", group-tuple form" : (p.form == MixForm::RowsSorted ? ", pattern-sorted objects" : (s.direct ? ", direct tables" : "")), p.ft, s.C);
}

}  // namespace sbe
