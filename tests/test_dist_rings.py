"""Several rings of overlap on the row-distributed solver (tuning dist_ras_rings), host side: nkp_dist_overlap_plan_host on CPU
over gloo.  The ring sets are computed here from the global matrix, the column coordinates and the partition; the plan must
build the hierarchy's matrix on [own rows | rings 1..r] in ascending global row order and an exchange that delivers exactly
those rows.  With one ring the plan must be the one-ring code's, field by field (recorded hashes, tests/golden)."""
import json
import os
import subprocess
import sys

import pytest

from test_dist_gloo import free_port

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ras_plan_depth1_sha256.json")


def launch(world, mode, out, extra=(), env_extra=None):
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
        env.pop("NKP_DIST_RAS_RINGS", None)
        env.pop("NKP_DIST_RAS", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_rings_worker.py"), "--mode", mode, "--out", out, *extra],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log
    return [json.load(open(f"{out}.{r}")) for r in range(world)]


def check_plan(res, rings):
    for r in res:
        print(r["rank"], "ring columns", r["ring_cols"], "overlap rows", r["n_sel"], "ras_need", r.get("ras_need"))
    assert all(r["ras"] == 1 and r["ras_rings"] == rings for r in res), res
    for r in res:
        assert r["n_sel"] == r["n_sel_expected"], r
        assert r["ext_matrix_ok"] and r["blocks_ok"] and r["coords_ok"] and r["sel_hpos_ok"] and r["ras_exchange_ok"], r
    # the rings do add rows: some rank has a second ring
    assert any(len(r["ring_cols"]) >= 2 and r["ring_cols"][1] > 0 for r in res), res


@pytest.mark.parametrize("rings", [2, 3])
@pytest.mark.parametrize("world,partition", [(2, "bands"), (3, "bands"), (2, "cells"), (3, "cells")])
def test_ring_plan_over_gloo(tmp_path, world, partition, rings):
    res = launch(world, "plan", str(tmp_path / "p"), extra=("--partition", partition, "--rings", str(rings)))
    check_plan(res, rings)


@pytest.mark.parametrize("rings", [2, 3])
def test_ring_plan_world_8_reaches_non_adjacent_bands(tmp_path, rings):
    """Thin bands: upwind3 reaches two latitude rows, so a deeper ring reaches owners two bands away; the plan must address
    them through the row starts."""
    res = launch(8, "plan", str(tmp_path / "p8"), extra=("--partition", "bands", "--grid", "24x40x8", "--rings", str(rings)))
    far = [r["rank"] for r in res if r["reaches_non_adjacent"]]
    print("ranks whose rings reach a non-adjacent band:", far)
    assert far, "precondition: on this grid some ring reaches a non-adjacent band"
    check_plan(res, rings)
    assert [r["rank"] for r in res if r["plan_reaches_non_adjacent"]] == far


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("rings", [-9, 0, 1])
@pytest.mark.parametrize("world,partition,grid", [(2, "bands", "24x20x10"), (3, "bands", "24x20x10"), (2, "cells", "24x20x10"),
                                                  (3, "cells", "24x20x10"), (2, "tracers", "24x20x10"), (8, "bands", "24x40x8")])
def test_depth_one_plan_equals_the_one_ring_plan(tmp_path, world, partition, grid, rings):
    """-9: tuning unset; 0: the caller's struct with the field zero-filled; 1: one ring asked for."""
    res = launch(world, "hash", str(tmp_path / "h"), extra=("--partition", partition, "--grid", grid, "--rings", str(rings)))
    want = _golden()[f"{world}-{partition}-{grid}"]
    for r in res:
        w = want[r["rank"]]
        assert r["ras"] == w["ras"], (r["rank"], r["ras"], w["ras"])
        for k, h in w["sha256"].items():
            assert r["sha256"][k] == h, (r["rank"], k, r["sizes"][k], w["sizes"][k])


GOLDEN_RINGS = os.path.join(HERE, "golden", "ras_plan_rings_sha256.json")
LAYOUTS = [(2, "bands", "24x20x10"), (3, "bands", "24x20x10"), (2, "cells", "24x20x10"), (3, "cells", "24x20x10"), (2, "tracers", "24x20x10"),
           (8, "bands", "24x40x8")]


def plan_record(res):
    """What the recorded file keeps of every rank's plan: the scalars, and per exported field the element count and the first
    16 hex digits of its SHA-256."""
    return [dict(scalars=r["scalars"], fields={k: [r["sizes"][k], h[:16]] for k, h in sorted(r["sha256"].items())}) for r in res]


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("world,partition,grid", LAYOUTS, ids=[f"{w}-{p}-{g}" for w, p, g in LAYOUTS])
def test_plan_equals_the_recorded_plan(tmp_path, world, partition, grid, depth):
    """Every exported field and scalar of every rank's plan at depths 1-3 against tests/golden/ras_plan_rings_sha256.json, which
    was recorded from the single-function planner that preceded csrc/dist_plan.cpp (with only its field table extended by
    origin / ship / ent_give / ent_need): the planner may be reshaped, the plan may not change."""
    res = launch(world, "hash", str(tmp_path / "h"), extra=("--partition", partition, "--grid", grid, "--rings", str(depth)))
    with open(GOLDEN_RINGS) as fh:
        want = json.load(fh)[f"{world}-{partition}-{grid}"][str(depth)]
    got = plan_record(res)
    assert len(got) == len(want) == world
    for rank, (g, w) in enumerate(zip(got, want)):
        assert g["scalars"] == w["scalars"], (rank, g["scalars"], w["scalars"])
        assert sorted(g["fields"]) == sorted(w["fields"]), rank
        for k in w["fields"]:
            assert g["fields"][k] == w["fields"][k], (rank, k, g["fields"][k], w["fields"][k])


def test_tracer_partition_gets_no_overlap_at_depth_3(tmp_path):
    res = launch(2, "plan", str(tmp_path / "t"), extra=("--partition", "tracers", "--grid", "24x20x10", "--rings", "3"))
    assert all(r["ras"] == 0 and r["n_sel"] == 0 and r["ras_rings"] == 0 and r["ring_cols"] == [] for r in res), res


@pytest.mark.parametrize("world", [2, 3])
def test_mismatched_requests_agree_on_the_minimum(tmp_path, world):
    res = launch(world, "mismatch", str(tmp_path / "m"), extra=("--rings", "2"))
    assert sorted({r["asked"] for r in res}) == [2, 3]
    check_plan(res, 2)


@pytest.mark.parametrize("value,bad_rank", [(5, -1), (-1, -1), (5, 1), (-3, 0)])
def test_out_of_range_depth_is_refused_on_every_rank(tmp_path, value, bad_rank):
    res = launch(2, "refuse", str(tmp_path / "x"), extra=("--grid", "24x20x10", "--rings", str(value), "--bad-rank", str(bad_rank)))
    for r in res:
        if r["bad"]:
            assert r["code"] == -1 and "dist_ras_rings" in r["message"], r          # NKP_EINVAL naming the field
        else:
            assert r["code"] == -5 and "failed its checks" in r["message"], r         # NKP_ECOMM naming the failing rank
