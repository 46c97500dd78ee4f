"""Worker for tests/test_gpu_stream_order.py: every device entry point on a caller's stream behind pending work, in a process of its
own (torch brings its own HIP runtime along).

The detector is a late producer.  An operand T of a library call is filled with NaN; then, on the stream S the solver was given,
a long sleep kernel, the copy of the true values into T and an event E are enqueued, and the library is called at once.  Whatever
reads T anywhere but in order on S -- another stream, the null stream, a synchronous copy before S is drained -- reads NaN.  E must
not have completed when the library is entered (recorded per call), and a control at the start shows that a reader on another
stream does see the NaN.  A result is read back on a stream that is not ordered with S, without any synchronisation of torch's.

One program of calls runs twice: first on fresh solvers that never see set_stream, every operand in place and
torch.cuda.synchronize () around every call (the expected bits), then on solvers put on S with every operand late.  The two runs
are compared by the bits of every result, the status and the iteration counts.  One JSON file."""
import argparse
import json
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

# as tests/test_gpu_step_glue.py: level 0 on the lane-per-column kernels, the levels below it one column per wave, a dense last level
GRID = dict(imt=24, jmt=20, km=12, adv="upwind3", hmix="isop", seed=4)
HIERARCHY = dict(ml_coarsest_rows=60, col_wave_max=300, col_ldsres_min=1)
SLEEP_MS = 30.0          # what the delay is scaled to; what decides is the per-call flag


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def summary(ret):
    """what a call answered with, in a form that compares by bits: status, iterations and relres of every right-hand side"""
    if ret is None:
        return None
    if isinstance(ret, dict):
        ret = [ret]
    if isinstance(ret, list) and all(isinstance(r, dict) for r in ret):
        return [[int(r["status"]), int(r["iters"]), float(r["relres"]).hex()] for r in ret]
    if isinstance(ret, list) and all(isinstance(r, int) for r in ret):
        return ret
    return None                                                     # tensors: they are compared as results


class Runner:
    """mode "expected": operands in place, torch.cuda.synchronize () before and after every call, results kept.
    mode "late": the producer of the module docstring in front of every call, results compared with the kept ones."""

    def __init__(self, torch, solver, system, mode, expected, cycles):
        self.torch, self.solver, self.system, self.mode, self.expected, self.cycles = torch, solver, system, mode, expected, cycles
        self.cases = []
        self.got = {}
        self.seen = set()
        self.armed = None
        self.entry_flag = None
        if mode == "late":
            self.S, self.S2, self.S3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        else:
            self.S = self.S2 = self.S3 = None
        self.default = torch.cuda.default_stream()

    # ---- tensors
    def dev(self, h):
        return self.torch.from_numpy(np.ascontiguousarray(h, np.float64)).cuda()

    def buf(self, like):
        return self.torch.zeros_like(like)

    # ---- solvers
    def make(self, kind, stream="S"):
        p, solver = self.system["p"], self.solver
        options = dict(self.system["coords"])
        if kind == "M":
            options.update(precond=solver.PRECOND_MULTILEVEL)
        else:
            options.update(precond=solver.PRECOND_COLUMN_JACOBI, basis_f32=1, max_iters=40)
        s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, self.system["blk"], tuning=dict(HIERARCHY), **options)
        if stream is not None:
            self.move(s, stream)
        return s

    def stream_of(self, key):
        return dict(S=self.S, S3=self.S3, default=self.default)[key]

    def move(self, s, key):
        """set_stream in the late run; the solvers of the expected bits never see it"""
        if self.mode == "late":
            s.set_stream(self.stream_of(key).cuda_stream)

    # ---- the hook of the wrapper's case: the flag is taken where the library is entered, inside torch's graph
    def hook(self, obj, names):
        for name in names:
            f = getattr(obj, name)

            def g(*args, _f=f, _name=name, **kw):
                if self.armed is not None:
                    self.entry_flag = not self.armed.query()
                    self.armed = None
                out = _f(*args, **kw)
                if _name == "transposed":
                    if not getattr(out, "_hooked", False):
                        out._hooked = True
                        self.hook(out, ["solve_batch_device"])
                return out
            setattr(obj, name, g)

    # ---- one call
    def late(self, case, name, entry, on, operand, pairs, fn, outs, stream="S"):
        """pairs: [(T, T_true)] the operands made late; fn: the call; outs: a list of tensors, or a function of fn's result that
        returns one.  Returns fn's result (None after an exception)."""
        torch = self.torch
        assert name not in self.seen, name
        self.seen.add(name)
        rec = dict(case=case, name=name, entry=entry, solver=on, operand=operand, error=None)
        ret = None
        try:
            with torch.no_grad():
                if self.mode == "expected":
                    for T, true in pairs:
                        T.copy_(true)
                    torch.cuda.synchronize()
                    unfinished = None
                else:
                    st = self.stream_of(stream)
                    for T, _ in pairs:
                        T.fill_(float("nan"))
                    torch.cuda.synchronize()
                    with torch.cuda.stream(st):
                        torch.cuda._sleep(self.cycles)
                        for T, true in pairs:
                            T.copy_(true, non_blocking=True)
                        E = torch.cuda.Event()
                        E.record(st)
            if self.mode == "expected":
                ret = fn()
                torch.cuda.synchronize()
                got = [o.detach().cpu().numpy().copy() for o in (outs(ret) if callable(outs) else outs)]
                self.expected[name] = dict(outs=got, ret=summary(ret))
            else:
                self.entry_flag, self.armed = None, E
                with torch.cuda.stream(st):
                    unfinished = not E.query()                      # immediately before the library is entered
                    ret = fn()
                    self.armed = None
                    if self.entry_flag is not None:                # the wrapper: where the first library call was made
                        unfinished = unfinished and self.entry_flag
                    results = outs(ret) if callable(outs) else outs
                # no synchronisation of torch's: the result is read on a stream that is not ordered with the solver's
                with torch.cuda.stream(self.S2), torch.no_grad():
                    copies = [o.detach().clone() for o in results]
                    self.S2.synchronize()
                    got = [c.cpu().numpy() for c in copies]
                torch.cuda.synchronize()
                want = self.expected.get(name)
                self.got[name] = got
                rec["unfinished_at_entry"] = bool(unfinished)
                if want is None:
                    rec["error"] = "the run of the expected bits has no such call"
                else:
                    differ = total = 0
                    for a, b in zip(got, want["outs"]):
                        total += b.size
                        differ += int(b.size) if a.shape != b.shape else int(np.count_nonzero(u64(a) != u64(b)))
                    rec.update(differ=differ, total=total, results=len(got), equal=bool(differ == 0 and len(got) == len(want["outs"])),
                               ret=summary(ret), ret_expected=want["ret"], ret_equal=summary(ret) == want["ret"])
        except Exception:
            self.armed = None
            rec["error"] = traceback.format_exc(limit=6)
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
        if self.mode == "late":
            self.cases.append(rec)
            print(f"case {case:2d} {name}: unfinished_at_entry={rec.get('unfinished_at_entry')} equal={rec.get('equal')} "
                  f"differ={rec.get('differ')}/{rec.get('total')} ret_equal={rec.get('ret_equal')} error={bool(rec['error'])}", flush=True)
        elif rec["error"]:
            self.expected[name] = dict(outs=[], ret=None, error=rec["error"])
            print(f"expected bits, case {case} {name}: {rec['error']}", flush=True)
        return ret


def hierarchy_kinds(s):
    """(wave_columns, lane_diag) of every smoothed level, and whether the last level is dense (tests/test_gpu_step_glue.py)"""
    nlev = s.get_int("levels")
    kinds = [(int(s.ml_level_array(l, "col_kernel")[0]), int(s.ml_level_array(l, "lane_diag")[0])) for l in range(nlev - 1)]
    return nlev, kinds, bool(s.ml_level_array(nlev - 1, "coarse_inv").size > 0)


def program(R, res):
    torch, solver = R.torch, R.solver
    p = R.system["p"]
    n, nnz = p.flat_len, int(p.colind.size)
    rng = np.random.default_rng(613)
    dev, buf = R.dev, R.buf
    vec = lambda *shape: dev(rng.standard_normal(shape))
    new = lambda like: torch.zeros_like(like)
    ptr = lambda t: t.data_ptr()
    # the solver's values times a fixed random factor in 0.9 .. 1.1: one factor for the whole matrix, which keeps every exact zero
    # of the hierarchy an exact zero, so that a refactor with flags 0 keeps the coarse cells
    values = lambda: dev(p.nzval * rng.uniform(0.9, 1.1))

    M, J = R.make("M"), R.make("J")
    if R.mode == "late":
        nlev, kinds, dense = hierarchy_kinds(M)
        res["hierarchy"] = dict(levels=nlev, kinds=kinds, dense_last=dense)
    handles = dict(M=M, J=J)

    # ---------------------------------------------------------------- 1: spmv_device
    x_true, xT, y = vec(n), buf(vec(n)), new(vec(n))
    R.late(1, "spmv late x", "spmv_device", "M", "x", [(xT, x_true)], lambda: M.spmv_device(ptr(xT), ptr(y)), [y])
    res.setdefault("spmv_x", x_true.cpu().numpy().tolist())

    # ---------------------------------------------------------------- 2: solve_device
    b_true, guess_true = vec(n), vec(n)

    def single_solves(case, s, on, tag, stream="S"):
        bT, x = buf(b_true), new(b_true)
        R.late(case, f"solve late b on {on}{tag}", "solve_device", on, "b", [(bT, b_true)],
               lambda: s.solve_device(ptr(bT), ptr(x), raise_on_fail=False), [x], stream)
        xT = buf(b_true)
        R.late(case, f"solve use_guess late x on {on}{tag}", "solve_device", on, "x", [(xT, guess_true)],
               lambda: s.solve_device(ptr(b_true), ptr(xT), use_guess=True, raise_on_fail=False), [xT], stream)
    for on in ("M", "J"):
        single_solves(2, handles[on], on, "")

    # ---------------------------------------------------------------- 3: solve_batch_device, K = 3
    B_true, G_true = vec(3, n), vec(3, n)

    def batched(case, s, on, tag, true=B_true, operand="B", stream="S"):
        BT, X = buf(true), new(true)
        R.late(case, f"solve_batch late {operand} on {on}, {tag}", "solve_batch_device", on, operand, [(BT, true)],
               lambda: s.solve_batch_device(ptr(BT), ptr(X), 3, n, raise_on_fail=False), [X], stream)
    for on in ("M", "J"):
        batched(3, handles[on], on, "first call (creates the members)")
        batched(3, handles[on], on, "existing members")

    # ---------------------------------------------------------------- 4: solve_batch_device_ex, a guess in column 1, per-column rtol
    X0_true = torch.zeros_like(B_true)
    X0_true[1] = guess_true
    ex = dict(rtol=[1e-6, None, 1e-8], use_guess=[False, True, False], raise_on_fail=False)
    BT, X = buf(B_true), X0_true.clone()
    R.late(4, "solve_batch_ex late B", "solve_batch_device_ex", "M", "B", [(BT, B_true)], lambda: M.solve_batch_device_ex(ptr(BT), ptr(X), 3, n, **ex), [X])
    XT = buf(B_true)
    R.late(4, "solve_batch_ex late X", "solve_batch_device_ex", "M", "X", [(XT, X0_true)], lambda: M.solve_batch_device_ex(ptr(B_true), ptr(XT), 3, n, **ex), [XT])

    # ---------------------------------------------------------------- 7: value_gradient_device, K = 2
    lam_true, x2_true, g_true = vec(2, n), vec(2, n), vec(nnz)
    lamT, g = buf(lam_true), new(g_true)
    R.late(7, "value_gradient late lam", "value_gradient_device", "M", "lam", [(lamT, lam_true)],
           lambda: M.value_gradient_device(ptr(lamT), ptr(x2_true), 2, n, ptr(g), alpha=-1.0), [g])
    x2T, g = buf(x2_true), new(g_true)
    R.late(7, "value_gradient late x", "value_gradient_device", "M", "x", [(x2T, x2_true)],
           lambda: M.value_gradient_device(ptr(lam_true), ptr(x2T), 2, n, ptr(g), alpha=-1.0), [g])
    gT = buf(g_true)
    R.late(7, "value_gradient accumulate late g", "value_gradient_device", "M", "g", [(gT, g_true)],
           lambda: M.value_gradient_device(ptr(lam_true), ptr(x2_true), 2, n, ptr(gT), alpha=-1.0, accumulate=True), [gT])

    # ---------------------------------------------------------------- 8: values_product_device and values_product_trans_device, K = 2
    v_true, y_true = dev(p.nzval * rng.standard_normal(nnz)), vec(2, n)

    def products(fn, entry, tags):
        vT, Y = buf(v_true), new(y_true)
        R.late(8, f"{entry} late val{tags[0]}", entry, "M", "val", [(vT, v_true)], lambda: fn(ptr(vT), ptr(x2_true), 2, n, ptr(Y), n, alpha=-1.0), [Y])
        xT2, Y2 = buf(x2_true), new(y_true)
        R.late(8, f"{entry} late x", entry, "M", "x", [(xT2, x2_true)], lambda: fn(ptr(v_true), ptr(xT2), 2, n, ptr(Y2), n, alpha=-1.0), [Y2])
        yT = buf(y_true)
        R.late(8, f"{entry} accumulate late y", entry, "M", "y", [(yT, y_true)],
               lambda: fn(ptr(v_true), ptr(x2_true), 2, n, ptr(yT), n, alpha=0.5, accumulate=True), [yT])
        if tags[1]:
            vT2, Y3 = buf(v_true), new(y_true)
            R.late(8, f"{entry} late val{tags[1]}", entry, "M", "val", [(vT2, v_true)], lambda: fn(ptr(vT2), ptr(x2_true), 2, n, ptr(Y3), n, alpha=-1.0), [Y3])
    products(M.values_product_device, "values_product_device", ("", None))
    index_before = M.get_int("trans_index_bytes")
    products(M.values_product_trans_device, "values_product_trans_device", (", first call (builds the index)", ", index exists"))
    if R.mode == "late":
        res["trans_index"] = dict(before=index_before, after=M.get_int("trans_index_bytes"))

    # ---------------------------------------------------------------- 9: solve_tangent_device, K = 2
    dval_true, db_true = dev(p.nzval * rng.standard_normal(nnz)), vec(2, n)
    for operand in ("dval", "x", "db"):
        T = dict(dval=buf(dval_true), x=buf(x2_true), db=buf(db_true))
        true = dict(dval=dval_true, x=x2_true, db=db_true)
        args = {k: (T[k] if k == operand else true[k]) for k in T}
        dX = new(db_true)
        R.late(9, f"solve_tangent late {operand}", "solve_tangent_device", "M", operand, [(T[operand], true[operand])],
               lambda: M.solve_tangent_device(ptr(args["dval"]), ptr(args["x"]), n, ptr(args["db"]), ptr(dX), 2, n, raise_on_fail=False), [dX])

    # ---------------------------------------------------------------- 5: refactor_device, then solves on the new matrix
    def refactor(tag, rebuild, after):
        val_true = values()
        vT = buf(val_true)
        flags = "rebuild" if rebuild else "flags 0"
        state = {}

        def call():
            M.refactor_device(ptr(vT), rebuild=rebuild)
            state["rebuilt"] = M.get_int("refactor_rebuilt")
            return [state["rebuilt"], M.get_int("refactor_count")]
        R.late(5, f"refactor {flags}, {tag}", "refactor_device", "M", "val", [(vT, val_true)], call, [])
        after(f"after refactor {flags}, {tag}")
        return state.get("rebuilt")

    def solve_after(tag):
        bT, x = buf(b_true), new(b_true)
        R.late(5, f"solve late b {tag}", "solve_device", "M", "b", [(bT, b_true)], lambda: M.solve_device(ptr(bT), ptr(x), raise_on_fail=False), [x])
    rebuilt = [refactor("no transposed handle", False, solve_after), refactor("no transposed handle", True, solve_after)]
    batched(5, M, "M", "members made again after the first rebuild")

    # ---------------------------------------------------------------- 6: transposed().solve_batch_device
    t = M.transposed()                                                  # built after set_stream
    batched(6, t, "transposed M", "handle built after set_stream", G_true, "G")
    M2 = R.make("M", stream=None)
    t2 = M2.transposed()                                                # built before set_stream
    R.move(M2, "S")
    batched(6, t2, "transposed M2", "handle built before set_stream", G_true, "G")
    M2.close()

    # ---------------------------------------------------------------- 5 again: the handle and its batch members alive
    def solves_after(tag):
        solve_after(tag)
        batched(5, M, "M", tag)
        batched(5, t, "transposed M", tag, G_true, "G")
    rebuilt += [refactor("transposed handle and members alive", False, solves_after), refactor("transposed handle and members alive", True, solves_after)]
    if R.mode == "late":
        res["refactor_rebuilt"] = rebuilt
        res["same_transposed_handle"] = M.transposed() is t

    # ---------------------------------------------------------------- 10: a clone is given the stream
    c = M.clone()
    state = {}
    try:
        R.move(c, "S")
        state["accepted"] = True
    except solver.NkpError as exc:
        state["accepted"] = str(exc)
    bT, x = buf(b_true), new(b_true)
    R.late(10, "solve late b on a clone of M", "solve_device", "clone of M", "b", [(bT, b_true)], lambda: c.solve_device(ptr(bT), ptr(x), raise_on_fail=False), [x])
    c.close()
    if R.mode == "late":
        res["clone_set_stream"] = state["accepted"]

    # ---------------------------------------------------------------- 11: the solver moves with members, handle and its members alive
    if R.mode == "late":
        res["before_move"] = dict(batch_member_bytes=M.get_int("batch_member_bytes"), transposed_batch_member_bytes=t.get_int("batch_member_bytes"))
    R.move(M, "S3")
    batched(11, M, "M", "moved to a third stream", stream="S3")
    batched(11, t, "transposed M", "moved to a third stream", G_true, "G", stream="S3")
    R.move(M, "default")
    single_solves(11, M, "M", ", moved to the default stream", stream="default")
    R.move(M, "S")

    # ---------------------------------------------------------------- 12: after an error
    nan_b, x = torch.full_like(b_true, float("nan")), new(b_true)
    torch.cuda.synchronize()
    with torch.cuda.stream(R.S) if R.mode == "late" else torch.no_grad():
        info = M.solve_device(ptr(nan_b), ptr(x), raise_on_fail=False)
    if R.mode == "late":
        res["nan_b_status"] = info["status"]
    bT, x = buf(b_true), new(b_true)
    R.late(12, "solve late b after a breakdown", "solve_device", "M", "b", [(bT, b_true)], lambda: M.solve_device(ptr(bT), ptr(x), raise_on_fail=False), [x])
    M.close()
    J.close()

    # ---------------------------------------------------------------- 13: the wrapper, on a third solver
    wrapper(R, res, vec, values)

    # ---------------------------------------------------------------- 14: a one-rank row-distributed solver on the file transport
    D, free = one_rank_distributed(R)
    try:
        single_solves(14, D, "one-rank row-distributed M", "")
        if R.mode == "late":
            res["one_rank_allreduce_calls"] = D.get_int("dist_allreduce_calls")      # 0 on a single-GPU solver
    finally:
        free()


def one_rank_distributed(R):
    """force_dist = 1 on the file transport, made as tests/test_gpu_step_glue.py makes it; returns the solver and what frees it"""
    import ctypes
    import tempfile
    solver, p = R.solver, R.system["p"]
    lib = solver.load_library()
    lib.nkp_comm_file_init.argtypes = [ctypes.POINTER(solver.NkpCommOps), ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.nkp_comm_file_free.argtypes = [ctypes.POINTER(solver.NkpCommOps)]
    lib.nkp_comm_file_free.restype = None
    rp, ci, v = np.ascontiguousarray(p.rowptr, np.int32), np.ascontiguousarray(p.colind, np.int32), np.ascontiguousarray(p.nzval, np.float64)
    blk = np.ascontiguousarray(R.system["blk"], np.int32)
    n = p.flat_len
    tmp = tempfile.TemporaryDirectory()
    ops = solver.NkpCommOps()
    if lib.nkp_comm_file_init(ctypes.byref(ops), tmp.name.encode(), 0, 1) != 0:
        raise RuntimeError("nkp_comm_file_init failed")
    opt = solver.default_options(precond=solver.PRECOND_MULTILEVEL)
    tun = solver.default_tuning(**dict(HIERARCHY, force_dist=1))
    opt.tuning = ctypes.pointer(tun)
    h = ctypes.c_void_p()
    rc = lib.nkp_create_dist(ctypes.byref(h), ctypes.byref(opt), n, 0, n, ci.size, solver._p(rp, ctypes.c_int32), solver._p(ci, ctypes.c_int32),
                             solver._p(v, ctypes.c_double), solver._p(blk, ctypes.c_int32), blk.size - 1, 1, ctypes.byref(ops))
    if rc != 0:
        raise RuntimeError(lib.nkp_last_error().decode())
    s = solver.NkpSolver._from_handle(lib, h, n, ci.size, opt)
    s._keep = (ops, tun, rp, ci, v, blk)
    R.move(s, "S")

    def free():
        s.close()
        lib.nkp_comm_file_free(ctypes.byref(ops))
        tmp.cleanup()
    return s, free


def wrapper(R, res, vec, values):
    """NkpTorchSolver constructed and used under torch.cuda.stream (S); the expected bits: the same program on the default stream"""
    import contextlib

    import torch.autograd.forward_ad as fwAD
    from nk_ocn_tracer_jacobian_precond_amd.torch_op import NkpTorchSolver
    torch = R.torch
    n = R.system["p"].flat_len
    K = 2
    under = (lambda: torch.cuda.stream(R.S)) if R.mode == "late" else contextlib.nullcontext
    M3 = R.make("M", stream=None)
    R.hook(M3, ["refactor_device", "solve_batch_device", "value_gradient_device", "values_product_device", "values_product_trans_device",
                "solve_tangent_device", "transposed"])
    with under():
        ts = NkpTorchSolver(M3)
    leaf = lambda true: torch.zeros_like(true).requires_grad_(True)
    val_true, B_true, W_true, P_true, dB_true = values(), vec(K, n), vec(K, n), vec(K, n), vec(K, n)
    q_true = val_true * vec(val_true.numel())

    val, B, W = leaf(val_true), leaf(B_true), torch.zeros_like(W_true)
    R.late(13, "wrapper set_values late val", "NkpTorchSolver.set_values", "M3", "val", [(val, val_true)], lambda: ts.set_values(val), [])
    X = R.late(13, "wrapper solve late B", "NkpTorchSolver.solve", "M3", "B", [(B, B_true)], lambda: ts.solve(B), lambda X: [X])
    if R.mode == "late":
        res["transposed_before_backward"] = getattr(M3, "_trans", None) is not None
    if X is not None:
        R.late(13, "wrapper backward late W", "backward of NkpTorchSolver.solve", "M3", "W", [(W, W_true)], lambda: X.mul(W).sum().backward(), lambda _: [B.grad, val.grad])
    if R.mode == "late":
        res["transposed_after_backward"] = getattr(M3, "_trans", None) is not None

    # the Hessian-vector product of tests/torch_second_order_worker.py (hessian_vector), P and q late where they enter
    val2, B2, W2 = leaf(val_true), leaf(B_true), leaf(W_true)
    P, q = torch.zeros_like(P_true), torch.zeros_like(q_true)
    with torch.no_grad():
        for T, true in ((val2, val_true), (B2, B_true), (W2, W_true)):
            T.copy_(true)
    torch.cuda.synchronize()
    with under():
        ts.set_values(val2)
        X2 = ts.solve(B2)
        gB, gval = torch.autograd.grad(X2.mul(W2).sum(), (B2, val2), create_graph=True)
    R.late(13, "wrapper Hessian-vector product late P and q", "double backward of NkpTorchSolver.solve", "M3", "P and q", [(P, P_true), (q, q_true)],
           lambda: torch.autograd.grad(gB.mul(P).sum() + gval.mul(q).sum(), (B2, val2, W2)), lambda h: list(h))

    # one forward-mode tangent
    dB = torch.zeros_like(dB_true)
    torch.cuda.synchronize()
    with fwAD.dual_level():
        with under():
            ts.set_values(val_true)
        R.late(13, "wrapper forward_ad late dB", "jvp of NkpTorchSolver.solve", "M3", "dB", [(dB, dB_true)],
               lambda: fwAD.unpack_dual(ts.solve(fwAD.make_dual(B_true, dB))), lambda d: [d.primal, d.tangent])
    torch.cuda.synchronize()
    M3.close()


def calibrate(torch, S):
    """cycles of torch.cuda._sleep for about SLEEP_MS on S, and what a sleep of that many cycles then measures"""
    def timed(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            e0.record(S)
            torch.cuda._sleep(cycles)
            e1.record(S)
        S.synchronize()
        return e0.elapsed_time(e1)
    timed(1000)
    probe = timed(10_000_000)
    cycles = max(1, int(10_000_000 * SLEEP_MS / probe))
    return cycles, probe, timed(cycles)


def control(torch, R, like):
    """the same poison, sleep and copy on S; a clone on a stream that does not wait for S must see the NaN"""
    T = torch.full_like(like, float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(R.S):
        torch.cuda._sleep(R.cycles)
        T.copy_(like, non_blocking=True)
        E = torch.cuda.Event()
        E.record(R.S)
    unfinished = not E.query()
    with torch.cuda.stream(R.S2):
        c = T.clone()
    torch.cuda.synchronize()
    return dict(unfinished_at_read=bool(unfinished), clone_saw_nan=bool(torch.isnan(c).any().item()), late_values_arrived=bool(torch.equal(T, like)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import oracle_binding as ora
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    torch.cuda.set_device(0)
    p = synth.generate(**GRID)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    system = dict(p=p, blk=solver.column_blocks(p.col_start(), p.tracer_state_len, 1), coords=dict(col_i=ci, col_j=cj))
    res = dict(n=int(p.flat_len), nnz=int(p.colind.size))

    expected = {}
    program(Runner(torch, solver, system, "expected", expected, 0), res)
    res["expected_errors"] = {k: v["error"] for k, v in expected.items() if v.get("error")}

    R = Runner(torch, solver, system, "late", expected, 0)
    R.cycles, res["probe_ms"], res["sleep_ms"] = calibrate(torch, R.S)
    res["sleep_cycles"] = R.cycles
    print(f"torch.cuda._sleep ({R.cycles}) measures {res['sleep_ms']:.2f} ms on the solver's stream", flush=True)
    res["control"] = control(torch, R, torch.randn(p.flat_len, dtype=torch.float64, device="cuda"))
    print("control:", res["control"], flush=True)
    program(R, res)
    res["cases"] = R.cases
    res["expected_calls"] = len(expected)

    # the anchor outside the library: the late-x product against the numpy oracle of the SpMV tests
    x = np.asarray(res.pop("spmv_x"), np.float64)
    y_ref = ora.spmv(p.rowptr, p.colind, p.nzval, x)
    y_late = R.got.get("spmv late x", [])
    res["spmv_late_x_has_the_oracle_bits"] = bool(len(y_late) == 1 and np.array_equal(u64(y_late[0]), u64(y_ref)) and np.abs(y_ref).max() > 0.0)
    with open(a.out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
