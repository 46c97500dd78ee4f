"""Matrices, kernel families and the kernel selection rule of the water-column band solves (csrc/colblock.hip and the lane
families csrc/col_lanes.hip, col_packed.hip, col_gs_fused.hip; the column kernels of csrc/batch.hip and csrc/mltail.hip) -- TEST
INFRASTRUCTURE.

Matrices.  widen(p, dists, seed) adds in-column entries at k +- d for every d in dists to a synth.generate problem: magnitude
0.02 |a_rr| U(0.5, 1), random sign, and the diagonal grows by the row sum of the added magnitudes with its own sign, so no
row's dominance margin inside its column block falls (the blocks of synth.generate are not row dominant to begin with).  dists = (3,) gives half bandwidth 3 (stored as 4 with one zero diagonal
each side), (4,) and (3, 4) give 4, (6,) and (3, 4, 6) give a measured band of 6: the band factors keep |row - col| <= 4 and
drop the rest (dropped = 1).  The low-order twin of the multilevel setup changes entries BETWEEN columns only, so level 0 of a
hierarchy keeps the in-column band of the matrix; the bands of the coarser levels are whatever the Galerkin products give
(the GPU tests read them from the device and record them).

Shapes.  The two grids of tests/test_gpu_colsolve_packed.py: 12 x 10, seed 36 (33 + 34 columns per colour: one full group of
32 and a last group of one or two; the longest column has exactly km rows) and 8 x 8, seed 7 (14 + 14: one partial group).

Families.  FAMILIES is one nkp_tuning dict per kernel.  Each sets col_stream_min = 1 and ml_coarsest_rows = 40, so that every
level but the last (which is solved densely) runs the kernel under test.

Selection rule.  expected_kernel restates col_plan (csrc/col_plan.cpp), the one place where the library decides which layout a
level gets and which instantiation serves it -- launch_colblock_apply_lanes, launch_colblock_apply_lanes_batch,
column_solves (csrc/mlcycle.hip) and finish_level_columns branch on its ColKernel.  tests/test_col_plan.py holds the two against each other
on the CPU; the GPU tests read the outcome through nkp_ml_level_array (.., "col_kernel").

  wave         only on a level without dropped entries (V.wave_columns)
  stream       only with columns of at most 64 rows
  packed       only with f32 storage, at most 80 rows, no fused sweep and no tail
  pipelined    only with f32, at most 64 rows, 8 columns per group, P <= 2 and at most 48 KB of LDS
  col_group    halved while (2 P + 2) * pad8 (max_len) * gw doubles exceed 56 KB
  lanes        <P, 64, ., 1> up to 64 rows, <P, 80, ., 3> up to 80 rows with col_w3, else <P, 128, ., 1>
  LDS          the dynamic LDS of the lane kernels; above 48 KB the setup opts in (hipFuncSetAttribute)

CASES_CYCLE / CASES_BATCH / CASES_REFACTOR / CASES_JACOBI are the case lists of tests/test_gpu_colsolve_families.py as data;
tests/test_colsolve_cases.py asserts from them and expected_kernel that every instantiation of INSTANTIATIONS is selected on
level 0 of at least one case (level 0 is the level whose band is known without a device)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import scipy.sparse as sp

from nk_ocn_tracer_jacobian_precond_amd import solver, synth

MAX_BAND = 4
GRID_BIG = (12, 10, 36)
GRID_SMALL = (8, 8, 7)
KMS = (10, 60, 64, 65, 80, 81, 96, 127, 128)

# in-column half bandwidth -> (adv, hmix, dists of widen)
BANDS = {1: ("centred", "const", ()), 2: ("upwind3", "isop", ()), 3: ("upwind3", "isop", (3,)), 4: ("upwind3", "isop", (3, 4)),
         6: ("upwind3", "isop", (3, 4, 6))}
BAND_ALTERNATIVES = {4: (4,), 6: (6,)}                 # further dists with the same measured band


# ---------------------------------------------------------------- matrices
def widen(p, dists, seed):
    """p with in-column entries added at k +- d for every d in dists (see the module docstring)."""
    if not dists:
        return p
    assert p.coupled_tracer_cnt == 1
    n = p.flat_len
    A = p.scipy_csr().tocoo()
    cs = np.asarray(p.col_start(), np.int64)
    col_of = np.repeat(np.arange(cs.size - 1), np.diff(cs))
    diag = p.scipy_csr().diagonal()
    assert (diag != 0).all()
    rng = np.random.default_rng(seed)
    rows, cols, vals = [A.row.astype(np.int64)], [A.col.astype(np.int64)], [A.data]
    grow = np.zeros(n)
    r_all = np.arange(n, dtype=np.int64)
    for d in dists:
        for side in (-1, 1):
            c = r_all + side * d
            ok = (c >= 0) & (c < n)
            ok[ok] = col_of[r_all[ok]] == col_of[c[ok]]
            mag = 0.02 * np.abs(diag) * rng.uniform(0.5, 1.0, n)
            sign = rng.choice(np.array([-1.0, 1.0]), n)
            rows.append(r_all[ok]); cols.append(c[ok]); vals.append((mag * sign)[ok])
            grow[ok] += mag[ok]
    rows.append(r_all); cols.append(r_all); vals.append(np.sign(diag) * grow)
    W = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    W.sum_duplicates()
    W.sort_indices()
    return dataclasses.replace(p, rowptr=W.indptr.astype(np.int32), colind=W.indices.astype(np.int32), nzval=W.data.astype(np.float64))


@functools.lru_cache(maxsize=None)
def problem(grid, km, band, dists=None):
    """The matrix of one case: synth.generate on the grid, widened to the in-column half bandwidth `band`."""
    imt, jmt, seed = grid
    adv, hmix, d = BANDS[band]
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv=adv, hmix=hmix, seed=seed)
    return widen(p, d if dists is None else dists, 1000 + band)


def column_blocks(p):
    return solver.column_blocks(p.col_start(), p.tracer_state_len, 1)


def column_dense_blocks(p, cap=None):
    """(first row, dense block) of every water column; cap: entries with |row - col| > cap removed."""
    A = p.scipy_csr()
    cs = np.asarray(p.col_start(), np.int64)
    out = []
    for a, b in zip(cs[:-1], cs[1:]):
        B = A[a:b, a:b].toarray()
        if cap is not None:
            i, j = np.indices(B.shape)
            B[np.abs(i - j) > cap] = 0.0
        out.append((int(a), B))
    return out


def dense_block_solve(p, r, cap=None):
    z = np.empty(p.flat_len)
    for a, B in column_dense_blocks(p, cap):
        z[a:a + B.shape[0]] = np.linalg.solve(B, r[a:a + B.shape[0]])
    return z


def fine_level_colour_lens(p):
    """Column lengths of level 0 per colour, in the order the lane layout groups them: colour (i + j) & 1 of the column's cell
    (ml_plan.cpp), the columns of a colour in their natural order."""
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    odd = ((np.asarray(ci) + np.asarray(cj)) & 1).astype(bool)
    lens = np.diff(np.asarray(p.col_start(), np.int64))
    return [lens[~odd], lens[odd]]


# ---------------------------------------------------------------- families
BASE = dict(col_stream_min=1, ml_coarsest_rows=40)
LAYOUTS = {
    "lanes8": dict(col_wave_max=0, col_stream=0, col_group=8),
    "stream32": dict(col_wave_max=0, col_stream=1, col_ldsres=0, col_stream_gw=32),
    "ldsres": dict(col_wave_max=0, col_ldsres=2, col_ldsres_packed=0, col_ldsres_early=0),
}
FAMILIES = {
    "wave2": dict(col_wave_max=10 ** 6, ml_wave_fused=0),
    "wave_fused": dict(col_wave_max=10 ** 6, ml_wave_fused=1),
    "lanes8": LAYOUTS["lanes8"],
    "lanes16": dict(col_wave_max=0, col_stream=0, col_group=16),
    "lanes32": dict(col_wave_max=0, col_stream=0, col_group=32),
    "lanes64": dict(col_wave_max=0, col_stream=0, col_group=64),
    "lanes8_now3": dict(LAYOUTS["lanes8"], col_w3=0),
    "lanes_pipe": dict(LAYOUTS["lanes8"], col_pipe_min=1),
    "stream32": LAYOUTS["stream32"],
    "stream64": dict(col_wave_max=0, col_stream=1, col_ldsres=0, col_stream_gw=64),
    "ldsres": LAYOUTS["ldsres"],
    "ldsres_early": dict(LAYOUTS["ldsres"], col_ldsres_early=1),
    "ldsres_long_only": dict(col_wave_max=0, col_ldsres=1),
    "ldsres_min": dict(col_wave_max=0, col_ldsres=2, col_ldsres_packed=0, col_ldsres_min=10 ** 6),   # no level has that many columns
    "packed_sorted": dict(col_wave_max=0, col_ldsres=2, col_ldsres_packed=1, col_sort_groups=1),
    "packed_unsorted": dict(col_wave_max=0, col_ldsres=2, col_ldsres_packed=1, col_sort_groups=0),
}
for _name, _layout in LAYOUTS.items():
    FAMILIES["gs_fused_" + _name] = dict(_layout, ml_fused=1)
    FAMILIES["tail_" + _name] = dict(_layout, ml_tail_rows=16000)
FAMILIES = {name: dict(BASE, **t) for name, t in FAMILIES.items()}
ANCHOR = "lanes8"

# the defaults of nkp_builtin_tuning (tuning.cpp) for the knobs the selection reads
TUNING_DEFAULTS = dict(col_ldsres=2, col_stream=1, col_stream_min=-1, col_stream_gw=32, col_wave_max=8192, col_w3=1, col_group=8,
                       col_pipe_min=0, col_ldsres_early=0, col_ldsres_packed=1, col_sort_groups=1, col_ldsres_min=0, ml_fused=0,
                       ml_wave_fused=1, ml_tail_rows=0)
LDSRES_CH = 16
GS_NNZ = 2048
GS_THREADS = 256
COL_KERNEL_FIELDS = ("wave_columns", "wave_fused", "stream", "ldsres", "gw", "P", "dropped", "max_len", "gs_ok", "ngrp", "lds_doubles")


def lds_pad(i):
    return i + (i >> 5)


def expected_kernel(family, f32, P, dropped, max_len, ncols, colour_lens=None, multilevel=True):
    """What a level with stored half bandwidth P, `dropped`, longest column max_len and ncols columns gets under
    FAMILIES[family] (a tuning dict is taken as it is): the fields of nkp_ml_level_array (.., "col_kernel") that follow from
    these arguments, `kernels` (the instantiations that serve single right-hand sides) and `batch` (K -> instantiations).
    colour_lens = the column lengths per colour in layout order: then ngrp, lds_doubles, gs_ok and lds_over_48k are exact;
    without it lds_over_48k is True / False where the bounds decide and None where they do not.  multilevel = False: the
    column-Jacobi preconditioner (one range, never wave, fused or tail; f32 = 0)."""
    T = dict(TUNING_DEFAULTS, **(FAMILIES[family] if isinstance(family, str) else family))
    f32 = bool(f32)
    fused_setup = multilevel and T["ml_fused"] != 0
    tail = multilevel and T["ml_tail_rows"] > 0
    ft = "f32" if f32 else "f64"
    # ---- col_plan: the layout
    gw = T["col_group"] if T["col_group"] in (8, 16, 32, 64) else 8
    on = T["col_stream"] != 0
    env_min = T["col_stream_min"] >= 0
    min_cols = T["col_stream_min"] if env_min else 50000
    stream = on and ncols >= min_cols and max_len <= 64
    if stream:
        gw = 64 if T["col_stream_gw"] == 64 else 32
    min_long, min_short = (min_cols, min_cols) if env_min else (8000, 20000)
    if T["col_ldsres_min"] > 0:
        min_long = min_short = T["col_ldsres_min"]
    lr = T["col_ldsres"]
    ldsres = int(lr > 0 and on and max_len <= 128 and ((max_len > 64 and ncols >= min_long) or (lr == 2 and ncols >= min_short)))
    if ldsres:
        stream, gw = False, 32
        if f32 and max_len <= 80 and T["col_ldsres_packed"] and not fused_setup and T["ml_tail_rows"] <= 0:
            ldsres = 2
    pad8 = (max_len + 7) & ~7
    while not stream and not ldsres and gw > 8 and (2 * P + 2) * pad8 * gw * 8 > 56 * 1024:
        gw >>= 1
    ndiag = 2 * P + 1
    in_lds = not stream and not ldsres                  # the lane kernel stages the factors in LDS
    m_pad = (max_len + LDSRES_CH - 1) // LDSRES_CH * LDSRES_CH if ldsres else pad8
    fac_doubles = ndiag * m_pad * gw                    # the group that holds the longest column
    fac_doubles = (fac_doubles + 1) // 2 if f32 else fac_doubles
    out = dict(stream=int(stream), ldsres=ldsres, gw=gw, P=P, dropped=int(bool(dropped)), max_len=max_len)
    sorted_groups = ldsres == 2 and T["col_sort_groups"] != 0
    if colour_lens is not None:
        need, ngrp = 0, 0
        for lens in colour_lens:
            lens = np.asarray(lens, np.int64)
            ngrp += (lens.size + gw - 1) // gw
            if not sorted_groups:
                for q in range(0, lens.size, gw):
                    need = max(need, lds_pad(int(lens[q:q + gw].sum())) + 2)
        if ldsres == 2:
            need = max(need, 32 * ((4 if max_len <= 64 else 5) * LDSRES_CH + 1))
        need = (need + 1) & ~1
        lds = need + (fac_doubles if in_lds else 0)
        gs_doubles = GS_NNZ + need + fac_doubles        # gs_fused_kernel stages the factors under every layout
        out.update(ngrp=ngrp, lds_doubles=lds, lds_over_48k=lds * 8 > 48 * 1024)
    else:
        lo = fac_doubles if in_lds else 0
        hi = lo + lds_pad(gw * max_len) + 3 + (32 * 81 if ldsres == 2 else 0)
        lds = None
        out.update(lds_over_48k=True if lo * 8 > 48 * 1024 else False if hi * 8 <= 48 * 1024 else None)
    # the fused half sweep: needs the row blocks (every row of these matrices is far below GS_NNZ entries) and 64 KB
    gs_ok = None
    if not fused_setup:
        gs_ok = 0
    elif sorted_groups:
        gs_ok = 0
    elif lds is not None:
        gs_ok = int(gs_doubles * 8 <= 64 * 1024)
    out["gs_ok"] = gs_ok
    # ---- col_plan: one column per wave (levels of the multilevel cycle)
    wave = multilevel and ncols <= T["col_wave_max"] and not dropped
    wf = T["ml_wave_fused"]
    wave_fused = wave and (wf == 1 or (wf > 1 and ncols <= wf))
    out.update(wave_columns=int(wave), wave_fused=int(wave_fused))
    # ---- col_plan: the instantiation launch_colblock_apply_lanes takes
    rpl = 1 if max_len <= 64 else 2
    if ldsres == 2:
        lanes = ("ldspack", P, 4 if max_len <= 64 else 5)
    elif ldsres:
        lanes = ("ldsres", P, ft, int(T["col_ldsres_early"] != 0))
    elif stream:
        lanes = ("stream", P, gw, ft)
    elif max_len <= 64:
        lanes = ("lanes", P, 64, ft)
    elif max_len <= 80 and T["col_w3"]:
        lanes = ("lanes", P, 80, ft)
    else:
        lanes = ("lanes", P, 128, ft)
    pipe_possible = f32 and max_len <= 64 and gw == 8 and P <= 2 and T["col_pipe_min"] > 0 and in_lds
    if pipe_possible and out["lds_over_48k"] is False:
        lanes = ("lanes_pipe", P)
    elif pipe_possible and out["lds_over_48k"] is None:
        lanes = None                                     # undecided without the column lengths
    if tail:
        kernels = {("tail", P, ft)}
    elif wave_fused:
        kernels = {("gs_wave", P, rpl, ft), ("wave", P, rpl, ft)}
    elif wave:
        kernels = {("wave", P, rpl, ft)}
    elif fused_setup and gs_ok:
        kernels = {("gs_fused", P, ft), lanes}
    elif fused_setup and gs_ok is None:
        kernels = set()
    else:
        kernels = {lanes}
    out["kernels"] = {k for k in kernels if k is not None}

    # ---- col_plan: batch4 / batch_other (the batched cycle has neither fused sweep nor tail)
    def batch(K):
        assert K in (2, 4, 8)
        if wave_fused:
            return {("gs_wave_batch", P, rpl), ("wave_batch", P, rpl)}
        if wave or ldsres != 2:
            return {("wave_batch", P, rpl)}
        return {("ldspack4" if K % 4 == 0 else "ldspack2", P, 4 if max_len <= 64 else 5)}
    out["batch"] = batch
    return out


def check_row_blocks(rowptr, r0, r1, starts):
    """The row blocks of the fused sweep (gs_fused_kernel) over the rows [r0, r1) of one group, given by their first rows:
    consecutive and covering, at most GS_THREADS rows and GS_NNZ entries each, and each as long as both limits allow."""
    rowptr = np.asarray(rowptr, np.int64)
    bounds = list(starts) + [r1]
    assert bounds[0] == r0 and all(a < b for a, b in zip(bounds[:-1], bounds[1:])), (r0, r1, bounds)
    for a, b in zip(bounds[:-1], bounds[1:]):
        assert b - a <= GS_THREADS and rowptr[b] - rowptr[a] <= GS_NNZ, (a, b)
        assert b == r1 or b - a == GS_THREADS or rowptr[b + 1] - rowptr[a] > GS_NNZ, (a, b)      # greedy-maximal


# Levels worked by hand: (family or tuning dict, f32, P, dropped, max_len, multilevel, field, value) on 67 columns; the field
# ("batch", K) is batch (K).  tests/test_colsolve_cases.py asserts them of expected_kernel, tests/test_col_plan.py of col_plan.
HAND_WORKED = [
    # wave only without dropped entries
    ("wave2", 1, 4, 0, 60, True, "kernels", {("wave", 4, 1, "f32")}),
    ("wave_fused", 0, 2, 0, 128, True, "kernels", {("gs_wave", 2, 2, "f64"), ("wave", 2, 2, "f64")}),
    ("wave2", 1, 4, 1, 60, True, "wave_columns", 0),
    ("wave2", 1, 4, 1, 60, True, "kernels", {("ldspack", 4, 4)}),       # ... falls to the default layout: packed with f32
    # stream only up to 64 rows
    ("stream32", 0, 2, 0, 64, True, "kernels", {("stream", 2, 32, "f64")}),
    ("stream64", 1, 1, 0, 64, True, "kernels", {("stream", 1, 64, "f32")}),
    ("stream32", 0, 2, 0, 65, True, "kernels", {("lanes", 2, 80, "f64")}),
    ("stream32", 0, 2, 0, 65, True, "gw", 8),
    # packed only with f32 storage, at most 80 rows, no fused sweep and no tail
    ("packed_sorted", 1, 2, 0, 80, True, "kernels", {("ldspack", 2, 5)}),
    ("packed_sorted", 1, 2, 0, 81, True, "kernels", {("ldsres", 2, "f32", 0)}),
    ("packed_sorted", 0, 2, 0, 80, True, "kernels", {("ldsres", 2, "f64", 0)}),
    (dict(FAMILIES["packed_sorted"], ml_fused=1), 1, 2, 0, 80, True, "ldsres", 1),
    (dict(FAMILIES["packed_sorted"], ml_tail_rows=16000), 1, 2, 0, 80, True, "ldsres", 1),
    # the pipelined kernel
    ("lanes_pipe", 1, 2, 0, 64, True, "kernels", {("lanes_pipe", 2)}),
    ("lanes_pipe", 1, 4, 0, 64, True, "kernels", {("lanes", 4, 64, "f32")}),
    ("lanes_pipe", 0, 2, 0, 64, True, "kernels", {("lanes", 2, 64, "f64")}),
    ("lanes_pipe", 1, 2, 0, 65, True, "kernels", {("lanes", 2, 80, "f32")}),
    # col_group halves against 56 KB: (2 P + 2) * pad8 (max_len) * gw * 8 bytes
    ("lanes64", 0, 1, 0, 10, True, "gw", 64),
    ("lanes64", 0, 1, 0, 60, True, "gw", 16),
    ("lanes64", 0, 2, 0, 60, True, "gw", 16),
    ("lanes64", 0, 4, 0, 60, True, "gw", 8),
    ("lanes64", 0, 4, 0, 128, True, "gw", 8),
    ("lanes32", 0, 1, 0, 56, True, "gw", 32),
    ("lanes32", 0, 1, 0, 57, True, "gw", 16),                            # 4 * 56 * 32 * 8 = 57344 = 56 KB
    # the lanes family's instantiations
    ("lanes8", 0, 4, 0, 80, True, "kernels", {("lanes", 4, 80, "f64")}),
    ("lanes8_now3", 0, 4, 0, 80, True, "kernels", {("lanes", 4, 128, "f64")}),
    ("lanes8", 1, 1, 0, 81, True, "kernels", {("lanes", 1, 128, "f32")}),
    # dynamic LDS: f64 factors of 9 diagonals x 128 rows x 8 columns alone are 72 KB
    ("lanes8", 0, 4, 0, 128, True, "lds_over_48k", True),
    ("lanes8", 1, 1, 0, 60, True, "lds_over_48k", False),
    # column-Jacobi: never wave, fused or tail
    ("wave2", 0, 4, 0, 60, False, "wave_columns", 0),
    # the batched cycle
    ("packed_sorted", 1, 4, 0, 80, True, ("batch", 2), {("ldspack2", 4, 5)}),
    ("packed_sorted", 1, 4, 0, 64, True, ("batch", 8), {("ldspack4", 4, 4)}),
    ("packed_sorted", 1, 4, 1, 81, True, ("batch", 4), {("wave_batch", 4, 2)}),
    ("wave_fused", 1, 4, 1, 60, True, ("batch", 4), {("ldspack4", 4, 4)}),
]
HAND_WORKED_NCOLS = 67


def batch_groups(width, rhs_batch=1):
    """The interleave widths K nkp_solve runs `width` right-hand sides with (a trailing single system is solved alone)."""
    kmax = 8 if rhs_batch >= 8 else 4 if (rhs_batch >= 4 or rhs_batch == 1) else 2
    out, left = [], width
    while left > 0:
        nact = min(left, kmax)
        if nact >= 2:
            out.append(2 if nact <= 2 else 4 if nact <= 4 else 8)
        left -= nact
    return out


def all_instantiations():
    """Every instantiation a launcher can select."""
    Ps, fts = (1, 2, 4), ("f32", "f64")
    inst = set()
    for P in Ps:
        for ft in fts:
            inst |= {("wave", P, rpl, ft) for rpl in (1, 2)} | {("gs_wave", P, rpl, ft) for rpl in (1, 2)}
            inst |= {("lanes", P, ml, ft) for ml in (64, 80, 128)}
            inst |= {("stream", P, gw, ft) for gw in (32, 64)}
            inst |= {("ldsres", P, ft, early) for early in (0, 1)}
            inst |= {("gs_fused", P, ft), ("tail", P, ft)}
        for nch in (4, 5):
            inst |= {("ldspack", P, nch), ("ldspack2", P, nch), ("ldspack4", P, nch)}
        for rpl in (1, 2):
            inst |= {("wave_batch", P, rpl), ("gs_wave_batch", P, rpl)}
        if P <= 2:
            inst.add(("lanes_pipe", P))
    return inst


INSTANTIATIONS = all_instantiations()

# ---------------------------------------------------------------- the case lists of tests/test_gpu_colsolve_families.py
# (b) the cycle: (grid, band, km, f32); every family of FAMILIES runs in every case
CASES_CYCLE = ([(GRID_BIG, band, km, f32) for band in (2, 4, 6) for km in (60, 80, 128) for f32 in (0, 1)]
               + [(GRID_BIG, band, km, f32) for band in (1, 3) for km in (10, 96) for f32 in (0, 1)]
               + [(GRID_SMALL, 4, km, f32) for km in (60, 128) for f32 in (0, 1)]
               + [(GRID_BIG, 1, 80, f32) for f32 in (0, 1)])        # P = 1 on 65 .. 80 rows: <1, 80, ., 3> and the 5-chunk packed kernel
# (c) batched solves: (grid, band, km, f32) x BATCH_FAMILIES x BATCH_WIDTHS
CASES_BATCH = ([(GRID_BIG, band, km, f32) for band in (2, 4, 6) for km in (60, 80, 128) for f32 in (0, 1)]
               + [(GRID_BIG, 1, km, 1) for km in (60, 80)])         # P = 1 through the packed batch kernels and the wave batch kernels
BATCH_FAMILIES = ("packed_sorted", "packed_unsorted", "ldsres", "lanes8", "wave2", "wave_fused")
BATCH_WIDTHS = ((2, 1), (3, 1), (4, 1), (5, 1), (6, 8), (8, 8))       # (width, rhs_batch)
CASES_BATCH_JACOBI = [(GRID_BIG, band, km) for band in (4, 6) for km in (60, 128)]
# (d) refactor: (grid, band, km) x REFACTOR_FAMILIES, f32 storage (packed needs it) and f64
CASES_REFACTOR = [(GRID_BIG, 4, km) for km in (60, 80)]
REFACTOR_FAMILIES = ("packed_sorted", "packed_unsorted", "ldsres", "stream32")
# (a) column-Jacobi against the oracle: (grid, band, km) x JACOBI_LAYOUTS
CASES_JACOBI = ([(GRID_BIG, band, km) for band in (1, 2, 3, 4, 6) for km in (10, 60, 64, 65, 80, 81, 128)]
                + [(GRID_SMALL, band, km) for band in (4, 6) for km in (60, 128)])
JACOBI_LAYOUTS = ("lanes8", "lanes16", "lanes32", "lanes64", "stream32", "stream64", "ldsres", "ldsres_early")


def stored_band(band):
    return 1 if band <= 1 else 2 if band <= 2 else 4


def level0(grid, band, km):
    """(P, dropped, max_len, ncols, colour_lens) of level 0 of the case's hierarchy, from the matrix alone."""
    p = problem(grid, km, band)
    lens = fine_level_colour_lens(p)
    return stored_band(band), int(band > MAX_BAND), int(max(l.max() for l in lens)), int(sum(l.size for l in lens)), lens


def covered_instantiations():
    """instantiation -> the cases whose LEVEL 0 selects it, over the case lists above; plus the two conditions on the layout."""
    hit = {}
    extra = dict(lanes_lds_over_48k=[], gs_fused_fallback=[])
    for grid, band, km, f32 in CASES_CYCLE:
        P, dropped, max_len, ncols, lens = level0(grid, band, km)
        for family in FAMILIES:
            e = expected_kernel(family, f32, P, dropped, max_len, ncols, lens)
            for k in e["kernels"]:
                hit.setdefault(k, []).append((family, grid, band, km, f32))
                if k[0] == "lanes" and e["lds_over_48k"] and "tail" not in family:
                    extra["lanes_lds_over_48k"].append((family, grid, band, km, f32))
            if family.startswith("gs_fused") and e["gs_ok"] == 0:
                extra["gs_fused_fallback"].append((family, grid, band, km, f32))
    for grid, band, km, f32 in CASES_BATCH:
        P, dropped, max_len, ncols, lens = level0(grid, band, km)
        for family in BATCH_FAMILIES:
            e = expected_kernel(family, f32, P, dropped, max_len, ncols, lens)
            for width, rhs_batch in BATCH_WIDTHS:
                for K in batch_groups(width, rhs_batch):
                    for k in e["batch"](K):
                        hit.setdefault(k, []).append((family, grid, band, km, f32, width))
    return hit, extra


REFACTOR_DIAGONAL_GROWTH = 0.10


def refactor_values(p, seed=77):
    """New values on p's pattern for the refactor cases: the diagonal grown by 10 % and every other in-column entry scaled by
    U(0.97, 1.03), so that every diagonal of every band factor changes; entries between columns stay.  (With the diagonal
    grown by 50 % or by 25 % the host planner picks other coarse cells on the last two levels of these shapes;
    tests/test_colsolve_cases.py checks with nkp_ml_plan_host that these values keep the cells.)"""
    cs = np.asarray(p.col_start(), np.int64)
    col_of = np.repeat(np.arange(cs.size - 1), np.diff(cs))
    row = np.repeat(np.arange(p.flat_len), np.diff(p.rowptr))
    col = np.asarray(p.colind, np.int64)
    val = np.array(p.nzval, np.float64, copy=True)
    inside = (col_of[row] == col_of[col]) & (row != col)
    val[inside] *= np.random.default_rng(seed).uniform(0.97, 1.03, int(inside.sum()))
    val[row == col] *= 1.0 + REFACTOR_DIAGONAL_GROWTH
    return val
