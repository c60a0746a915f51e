"""The numbers the three matrix-pipe units share (sbayes_amd/csrc/sbe_tile_plan.h: sbe_assoc, sbe_consensus, sbe_partdist)
without a GPU.  tests/c/tile_plan.cpp includes only that header; it is built with AddressSanitizer + UBSan (a stand-alone
binary: nothing is preloaded; without the sanitizer runtimes it is built plain and the log says so) and asked questions on
stdin.  The figures asserted are the ones the units' comments and DESIGN.md section 13 state."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
ROUND, TILE = 256, 32
# the longest enumeration of tile pairs any unit has: sbe_assoc at 4096 features of 32 states, a feature a tile
MOST_TILES = 4096
# each unit's longest contraction axis and most rows: sbe_assoc 2^24 objects; sbe_consensus and sbe_partdist 16384 objects
# and 2^20 samples of 8 clusters per run
LARGEST = (1 << 24, 16384, (1 << 20) * 8)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tile_plan") / "tile_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", str(REPO / "tests" / "c" / "tile_plan.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        print("[tile_plan] sanitizer runtimes not installed: built WITHOUT -fsanitize=address,undefined")
        build = subprocess.run([c for c in cmd if not c.startswith("-fsanitize")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]

    def ask(questions):
        run = subprocess.run([str(exe)], input="".join(q + "\n" for q in questions), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
        out = [json.loads(line) for line in run.stdout.splitlines()]
        assert len(out) == len(questions)
        return out

    return ask


def test_geometry(ask):
    g = ask(["geometry"])[0]
    assert (g["tile"], g["step"], g["round"], g["round_elems"], g["round_bytes"], g["acc_regs"]) == (TILE, 64, 4, ROUND, ROUND // 2, 16)
    assert g["acc_regs"] * 64 == g["tile"] ** 2                      # 64 lanes hold the tile
    assert (g["steps_per_launch"], g["max_launch_tiles"]) == (1 << 22, 1 << 16)


def test_tile_pair_inverts_the_triangular_enumeration(ask):
    total = MOST_TILES * (MOST_TILES + 1) // 2
    got = ask([f"pairs {total}"])[0]
    assert got == {"checked": total, "wrong": 0, "first_wrong": -1, "last_J": MOST_TILES - 1}


def test_accumulator_rows_are_a_permutation_of_the_tile_rows(ask):
    rows = ask(["acc"])[0]["rows"]
    assert len(rows) == 32 and sorted(rows) == list(range(TILE))
    assert rows[0] == 0 and rows[16] == 4                            # register 0 of half 0, of half 1
    assert rows[:8] == [0, 1, 2, 3, 8, 9, 10, 11] and rows[16:20] == [4, 5, 6, 7]


def test_tiles_per_launch(ask):
    steps = [1, 1 << 18, (1 << 18) + 1, 1 << 22, (1 << 22) + 1, 1 << 30]
    got = [a["tiles"] for a in ask([f"launch {s} 0" for s in steps])]
    assert got == [1 << 16, 16, 15, 1, 1, 1]
    assert [a["tiles"] for a in ask([f"launch {s} {o}" for s in steps for o in (1, 7, 1 << 16)])] == [1, 7, 1 << 16] * len(steps)


def test_whole_rounds_and_tiles(ask):
    ns = (1, 255, 256, 257) + LARGEST + tuple(n - 1 for n in LARGEST) + tuple(n + 1 for n in LARGEST)
    for n, got in zip(ns, ask([f"pad {n}" for n in ns])):
        assert got["rounds"] == -(-n // ROUND) and got["whole_rounds"] == got["rounds"] * ROUND, (n, got)
        assert got["tiles"] == -(-n // TILE) and got["whole_tiles"] == got["tiles"] * TILE, (n, got)
        assert 0 <= got["whole_rounds"] - n < ROUND and 0 <= got["whole_tiles"] - n < TILE, (n, got)
    first = dict(zip(ns, ask([f"pad {n}" for n in ns[:4]])))
    assert [first[n]["whole_rounds"] for n in (1, 255, 256, 257)] == [256, 256, 256, 512]
    assert [first[n]["whole_tiles"] for n in (1, 255, 256, 257)] == [32, 256, 256, 288]
