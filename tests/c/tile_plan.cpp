// tile_plan.cpp -- the numbers of the matrix-pipe units (sbayes_amd/csrc/sbe_tile_plan.h) without a GPU: reads one question
// per line from stdin and prints one JSON line per question (tests/test_tile_plan_cpu.py).
//   geometry            the constants
//   pairs T             tile_pair(t) for every t < T against the enumeration walked pair by pair: how many differ, the first
//   acc                 acc_row(reg, half) for half 0 then half 1, reg 0 .. 15
//   launch STEPS TILES  tiles_per_launch(STEPS, TILES)
//   pad N               rounds_of, whole_rounds, tiles_of, whole_tiles of N
#include "../../sbayes_amd/csrc/sbe_tile_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace sbe_tile;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream words(line);
        std::string what;
        long long a = 0, b = 0;
        if (!(words >> what)) continue;
        words >> a >> b;
        if (what == "geometry") {
            std::printf("{\"tile\": %d, \"step\": %d, \"round\": %d, \"round_elems\": %d, \"round_bytes\": %d, \"acc_regs\": %d, \"steps_per_launch\": %lld, "
                        "\"max_launch_tiles\": %lld}\n", kTile, kStep, kRound, kRoundElems, kRoundBytes, kAccRegs, (long long)kStepsPerLaunch,
                        (long long)kMaxLaunchTiles);
        } else if (what == "pairs") {
            long long wrong = 0, first = -1;
            int64_t I = 0, J = 0;                                  // the pair of t, walked: I runs to J, then the next J
            for (int64_t t = 0; t < a; ++t) {
                const TilePair p = tile_pair(t);
                if (p.I != I || p.J != J || J * (J + 1) / 2 + I != t) {
                    if (wrong++ == 0) first = (long long)t;
                }
                if (++I > J) { I = 0; ++J; }
            }
            std::printf("{\"checked\": %lld, \"wrong\": %lld, \"first_wrong\": %lld, \"last_J\": %lld}\n", a, wrong, first, (long long)tile_pair(a - 1).J);
        } else if (what == "acc") {
            std::printf("{\"rows\": [");
            for (int half = 0; half < 2; ++half)
                for (int reg = 0; reg < kAccRegs; ++reg) std::printf("%s%d", half + reg ? ", " : "", acc_row(reg, half));
            std::printf("]}\n");
        } else if (what == "launch") {
            std::printf("{\"tiles\": %lld}\n", (long long)tiles_per_launch(a, b));
        } else if (what == "pad") {
            std::printf("{\"rounds\": %lld, \"whole_rounds\": %lld, \"tiles\": %lld, \"whole_tiles\": %lld}\n", (long long)rounds_of(a), (long long)whole_rounds(a),
                        (long long)tiles_of(a), (long long)whole_tiles(a));
        } else {
            std::fprintf(stderr, "bad question: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
