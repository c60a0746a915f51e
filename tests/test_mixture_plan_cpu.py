"""The launch decision of the fused mixture kernel (sbayes_amd/csrc/sbe_mixture_plan.h: plan_mixture) without a GPU.
tests/c/mixture_plan.cpp includes only that header; it is built with AddressSanitizer + UBSan (a stand-alone binary: nothing is
preloaded; without the sanitizer runtimes it is built plain and the log says so) and fed cases on stdin.  Two kinds of
cases: anchors that the GPU suite and the measured-threshold comments already state, and the record of what the engine
chose on an MI355X at the commit before the planner existed (tests/golden/mixture_plan_parent.json, written by
tools/diag/mixture_plan_sweep.py): the planner must give every recorded name or refusal back, character for character."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
RECORD = REPO / "tests" / "golden" / "mixture_plan_parent.json"
OPTIONS = {"packed": 0, "onehot": 1, "packed_general": 2, "packed_tuple": 3, "onehot_general": 4, "packed_tuple_lds": 5,
           "packed_v2": 6, "packed_tuple_mfma": 7}
MFMA, TUPLE64, COMBO, ROWS, ROWS_SORTED, ONEHOT_V2, V2 = range(7)          # MixForm
ERR_ARG, ERR_STATE = 1, 3
HEADLINE = dict(N=1000, F=200, S=10, C=2, Gtot=6, slots=4096, cu=256, P=2, KT=6, share_ok=1, waits=1)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mixture_plan") / "mixture_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", str(REPO / "tests" / "c" / "mixture_plan.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        print("[mixture_plan] sanitizer runtimes not installed: built WITHOUT -fsanitize=address,undefined")
        build = subprocess.run([c for c in cmd if not c.startswith("-fsanitize")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]

    def plan(cases):
        text = "".join(" ".join(f"{k}={int(v)}" for k, v in c.items()) + "\n" for c in cases)
        run = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
        out = [json.loads(line) for line in run.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return plan


def test_headline_thresholds(planner):
    ns = (31, 32, 319, 512, 513, 576, 1024, 4096)
    got = dict(zip(ns, planner([dict(HEADLINE, n=n) for n in ns])))
    assert got[31]["text"] == "k_mixture_tuple64<packed stream, group-tuple form, tile 64, C=2>" and got[31]["form"] == TUPLE64
    for n in (32, 319, 512):
        assert got[n]["text"] == "k_mixture_tuple_mfma<packed stream, group-tuple form, matrix pipe fp4, 4 slots x M tiles 1, C=2>", (n, got[n])
        assert (got[n]["form"], got[n]["SL"], got[n]["MT"], got[n]["in_kernel"]) == (MFMA, 4, 1, 1)
    for n in (513, 576, 1024, 4096):
        assert got[n]["text"] == "k_mixture_tuple_mfma<packed stream, group-tuple form, matrix pipe fp4, 16 slots x M tiles 3, C=2, shared operands>", (n, got[n])
    assert (got[4096]["n_split"], got[4096]["grid"], got[4096]["n_partials"]) == (1, 256, 1)
    unshared = planner([dict(HEADLINE, n=n, share_ok=0) for n in (513, 576, 1024, 4096)])
    for p in unshared:
        assert p["text"] == "k_mixture_tuple_mfma<packed stream, group-tuple form, matrix pipe fp4, 16 slots x M tiles 3, C=2>", p
    assert "shared operands" not in planner([dict(HEADLINE, n=1024, shared=0)])[0]["text"]


def test_units_of_the_four_slot_against_the_sixteen_slot_form(planner):
    """1 / 1 / 2 / 2 units against 3 at 32 / 256 / 320 / 512 headline states, 4 against 3 at 576 (the comment in mfma_geometry)."""
    ns = (32, 256, 320, 512, 576)
    got = planner([dict(HEADLINE, n=n, kernel=OPTIONS["packed_tuple_mfma"]) for n in ns])
    assert [(p["units4"], p["units16"]) for p in got] == [(1, 3), (1, 3), (2, 3), (2, 3), (4, 3)]
    assert [p["SL"] for p in got] == [4, 4, 4, 4, 16]
    assert [p["SL"] for p in planner([dict(HEADLINE, n=n, kernel=OPTIONS["packed_tuple_mfma"], small_sl4=0) for n in ns])] == [16] * 5


def test_overflow_guard_of_the_exponent_sums(planner):
    """test_exponent_sums_close_under_the_overflow_guard: 57 passes in one split are planned, 58 refused, 58 without the override planned."""
    case = dict(N=8900, S=2, C=1, Gtot=4, slots=1, cu=256, n=1, P=1, KT=4, kernel=OPTIONS["packed_tuple_mfma"], waits=1)
    ok, refused, free = planner([dict(case, F=14560, split=1), dict(case, F=14593, split=1), dict(case, F=14593)])
    assert ok["text"] == "k_mixture_tuple_mfma<packed stream, group-tuple form, matrix pipe fp4, 4 slots x M tiles 1, C=1>"
    assert (ok["n_split"], ok["nt_per_split"]) == (1, 910) and -(-ok["nt_per_split"] // 16) == 57
    assert refused["err"] == ERR_ARG and refused["text"].startswith("matrix-pipe group-tuple kernel forced but not applicable (tuples=4, C=1, LDS ")
    assert free["err"] == 0 and free["form"] == MFMA and free["n_split"] > 1
    for kt in (1, 8):
        assert planner([dict(case, F=14560, split=1, KT=kt)])[0]["err"] == 0


def test_wide_forms_and_the_lds_fallback(planner):
    # 16 tuples in 4 slots per block pad to 2 M tiles x 8 tuples: 200 objects are fewer than 16 per padded tuple
    wide = dict(N=200, F=200, S=10, C=3, Gtot=7, slots=1024, cu=256, n=512, P=4, KT=16, waits=1)
    default, forced, shared_enough = planner([wide, dict(wide, kernel=OPTIONS["packed_tuple_mfma"]), dict(wide, wide_min_share=0)])
    assert default["form"] != MFMA and default["err"] == 0
    for p in (forced, shared_enough):
        assert p["text"] == "k_mixture_tuple_mfma<packed stream, group-tuple form, matrix pipe fp4, 4 slots x M tiles 2, C=3>", p
    # 5000 objects x 6 tuples: the A image of 16 slots (3 M tiles x 80 KB) does not fit LDS, that of 4 slots does
    big = planner([dict(HEADLINE, N=5000, n=1024)])[0]
    assert (big["form"], big["SL"], big["MT"]) == (MFMA, 4, 1) and 80 * 1024 < big["lds"] <= 160 * 1024


def test_one_case_for_each_remaining_form(planner):
    s130 = dict(N=300, F=40, S=130, C=2, Gtot=4, slots=64, cu=256, n=8, P=2, KT=4, waits=1)
    # (47 tables of 10 states: 84 KB at 32 features with the weights and 8 KB of ids, over the 78 KB of two blocks per CU -> v2 tile 16)
    c4 = dict(N=5000, F=200, S=10, C=4, Gtot=46, slots=320, cu=256, P=8, KT=0, waits=1)
    direct = dict(N=300, F=48, S=40, C=3, Gtot=66, slots=64, cu=256, n=8, P=4, KT=0, waits=1)
    got = planner([dict(s130, kernel=OPTIONS["packed_tuple"]), dict(c4, n=15, kernel=OPTIONS["packed_general"]),
                   dict(c4, n=16, kernel=OPTIONS["packed_general"]), dict(c4, n=64), dict(c4, n=8),
                   dict(c4, n=8, kernel=OPTIONS["onehot_general"]), dict(c4, n=64, kernel=OPTIONS["packed_v2"]), direct,
                   dict(c4, n=8, kernel=OPTIONS["packed_tuple"]), dict(c4, n=15, kernel=OPTIONS["packed_general"], rows_sorted=2)])
    assert got[0]["text"] == "k_mixture_combo<packed stream, group-tuple form, tile 16, C=2>" and got[0]["form"] == COMBO and got[0]["state_h"] == 0
    assert got[1]["text"] == "k_mixture_rows<packed stream, tile 32, C=4>" and got[1]["form"] == ROWS
    assert got[2]["text"] == "k_mixture_rows<packed stream, pattern-sorted objects, tile 32, C=4>" and got[2]["form"] == ROWS_SORTED
    assert got[3]["form"] == ROWS_SORTED and got[4]["form"] == V2          # packed: 64 x 5000 x 200 observations reach the rows form, 8 do not
    assert got[5]["text"] == "k_mixture_onehot_v2<one-hot stream, tile 16, C=4>" and got[5]["form"] == ONEHOT_V2
    assert got[6]["text"] == "k_mixture_v2<packed stream, tile 16, C=4>" and got[6]["form"] == V2
    assert got[7]["text"] == "k_mixture_v2<packed stream, direct tables, tile 16, C=3>" and got[7]["direct"] == 1
    assert got[8]["err"] == ERR_ARG and got[8]["text"] == "group-tuple kernel forced but not applicable (tuples=0, LDS 0 bytes)"
    assert got[9]["form"] == ROWS_SORTED


def test_refusals_of_hand_made_shapes(planner):
    """The two refusals no created engine reaches: tables that creation would have gathered directly, a partials buffer of one entry."""
    direct = dict(N=300, F=48, S=40, C=3, Gtot=66, slots=64, cu=256, n=8, P=4, KT=0, waits=1)
    lds, partials = planner([dict(direct, o_direct=0), dict(HEADLINE, n=1, o_partials=1)])
    assert lds["err"] == ERR_ARG and lds["text"].startswith("probability / weight tables too large for LDS staging at tile width 16 (")
    assert lds["text"].endswith("bytes; G_total=66, S=40, P=4)")
    assert partials["err"] == ERR_STATE and partials["text"].startswith("internal: partials buffer too small (") and partials["text"].endswith(" > 1)")
    assert planner([dict(direct, ft=64)])[0] == {"shape_refused": True}          # SBE_FT=64: sbe_create's own refusal


def test_where_the_final_reduction_runs(planner):
    one_block = dict(N=50, F=30, S=5, C=2, Gtot=3, slots=1024, cu=256, n=1024, P=2, KT=0)   # 13 quads, one tile: one block when 1024 slots fill the chip
    few = dict(HEADLINE, n=31)                       # 16 blocks per slot
    many = dict(HEADLINE, n=1)                       # hundreds of blocks per slot
    got = planner([dict(HEADLINE, n=1024), dict(HEADLINE, n=1024, epilogue=1), dict(HEADLINE, n=1024, in_kernel=0),
                   dict(one_block, waits=1), dict(few, waits=0), dict(few, waits=1), dict(many, waits=0), dict(few, waits=0, epilogue=1)])
    assert [p["n_partials"] for p in got[3:7]] == [1, 16, 16, got[6]["n_partials"]] and got[6]["n_partials"] > 16
    assert [p["in_kernel"] for p in got] == [1, 0, 0, 1, 1, 0, 0, 0]
    assert got[0]["done_blocks"] == 1024 // 16 and got[3]["done_blocks"] == 1024 and got[4]["done_blocks"] == 31


def test_planner_reproduces_the_parent_record(planner):
    """Record lines: {"job": ...} with what a process' launches share, then per launch
    [option, n, P, KT, share_ok, name or refusal, error code, digest of the results]."""
    cases, want = [], []
    for rec in map(json.loads, RECORD.read_text().splitlines()):
        if isinstance(rec, dict):
            job = rec["job"]
            n_obj, n_feat, n_states, groups, slots = job["create"]
            env = dict(job["env"])
            shared = dict(N=n_obj, F=n_feat, S=n_states, C=len(groups), Gtot=sum(groups), slots=slots, cu=job["compute_units"], waits=1)
            for name, key in (("SBE_ROWS_SORTED", "rows_sorted"), ("SBE_MFMA_SPLIT", "split"), ("SBE_MFMA_WIDE_MIN_SHARE", "wide_min_share")):
                if name in env:
                    shared[key] = int(env.pop(name))
            if "SBE_MFMA_SMALL_SL4" in env:
                shared["small_sl4"] = int(env.pop("SBE_MFMA_SMALL_SL4")) != 0
            assert not env, env                      # a variable this test does not hand to the planner
            continue
        option, n, n_patterns, n_tuples, share_ok, text, code, _digest = rec
        cases.append(dict(shared, kernel=OPTIONS[option], n=n, P=n_patterns, KT=n_tuples, share_ok=share_ok))
        want.append((text, code))
    assert len(cases) > 500
    wrong = [(c, w, p) for c, w, p in zip(cases, want, planner(cases)) if (p.get("text"), p.get("err")) != w]
    assert not wrong, (len(wrong), wrong[:3])
