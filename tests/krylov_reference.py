"""The Krylov drivers of csrc/krylov.hip restated in numpy -- TEST INFRASTRUCTURE.

fgmres () restates fg_begin, fg_restart, arnoldi_apply, arnoldi_orthogonalise, fg_post_step and fg_end_cycle (csrc/krylov.hip,
with their host arithmetic in csrc/krylov_host.cpp: fg_restart_verdict, fg_column_step, fg_back_substitute) together with the
column epilogues of csrc/blas1.hip:418-486; bicgstab () restates bicgstab of csrc/krylov.hip.  Vectors are float64; every inner product and norm is accumulated in np.longdouble and rounded
once (Arith).  The operator A and the preconditioner M are callables on float64 vectors, so the same text runs on the oracle's
operators (tests/test_krylov_reference.py) and on the solver's own spmv / precond_apply (tests/test_gpu_krylov.py).

Both drivers begin with the verdict on the right-hand side (rhs_verdict of csrc/krylov_host.cpp restated: NaN, Inf and norms
outside the range of a solve are refused with x = NaN) and treat a non-finite residual norm as a breakdown; berr () restates the
NaN-sticky backward-error reduction of csrc/blas1.hip.

A solve cut at max_iters = k returns x_k, which GMRES fixes uniquely (the residual minimiser over the Krylov space): two correct
implementations agree on it to rounding, whatever their summation order.

Every host decision of the drivers is logged with the relative distance of the two numbers compared (Result.log), so that a
test can show that no decision of a case sits within rounding of its threshold.  fgmres (trace=[...]) also records what the
host saw and made of it, in order: ("restart", beta), then if the solve goes on ("cycle", steps_now, stalled_cycles,
inner_scale); per step ("step", h, its, est, ends) with the Hessenberg column as it came from the device (est None: breakdown);
per cycle ("end", k, y, cs, sn, g, columns of the rotated H) -- the input and the expected decisions of tests/test_krylov_host.py.

Arith is the seam for the variants of tests/test_krylov_reference.py: plain f64 accumulation in reversed order (what two
correct implementations differ by) and three deliberately wrong ones (what the GPU tests must be able to see).
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

OK, NOT_CONVERGED, BREAKDOWN, OK_BERR = 0, 1, 2, 3
LD = np.longdouble

Result = namedtuple("Result", "x iters status relres log stagnated inner_scale")
Decision = namedtuple("Decision", "kind its lhs rhs taken dist")


class Arith:
    """The vector arithmetic of csrc/blas1.hip with longdouble accumulation."""

    def dot(self, x, y):
        """dot_kernel / multi_dot_body (blas1.hip:47-140, 349-373): sum x_i y_i"""
        return float(np.dot(np.asarray(x, LD), np.asarray(y, LD)))

    def sumsq(self, h):
        """finish_column_pythagoras_body (blas1.hip:442-456): sum h_j^2"""
        h = np.asarray(h, LD)
        return float(np.dot(h, h))

    def update(self, w, V, h, sign=-1.0):
        """update_w_body (blas1.hip:151-192): w += sign * sum_j h[j] V[j], one vector after the other in f64"""
        w = w.copy()
        for j in range(len(V)):
            w += (sign * h[j]) * np.asarray(V[j], np.float64)
        return w

    def scale_to(self, w, a, f32):
        """scale_to_body (blas1.hip:255-272): y = a w, and the f32 copy of y (not of w)"""
        y = a * w
        return y, (y.astype(np.float32) if f32 else None)


class ReversedF64(Arith):
    """Plain f64 accumulation, one element after the other from the last to the first."""

    def dot(self, x, y):
        p = (np.asarray(x, np.float64) * np.asarray(y, np.float64))[::-1]
        return float(np.cumsum(p)[-1]) if p.size else 0.0

    def sumsq(self, h):
        return self.dot(h, h)

    def update(self, w, V, h, sign=-1.0):
        w = w.copy()
        for j in reversed(range(len(V))):
            w += (sign * h[j]) * np.asarray(V[j], np.float64)
        return w


# ---- the verdict on the right-hand side (csrc/krylov_host.cpp: rhs_needs_counts, rhs_verdict; include/nkp.h at nkp_solve)
TARGET_FLOOR = 2.0 ** -480
RHS_ORDINARY, RHS_ZERO, RHS_NONFINITE, RHS_OUT_OF_RANGE = 0, 1, 2, 3


def rhs_needs_counts(bnorm2, target):
    return not math.isfinite(bnorm2) or not target >= TARGET_FLOOR


def rhs_verdict(bnorm2, target, n_nonfinite, n_nonzero):
    if not rhs_needs_counts(bnorm2, target):
        return RHS_ORDINARY if bnorm2 > 0.0 else RHS_ZERO
    if n_nonfinite != 0:
        return RHS_NONFINITE
    return RHS_ZERO if n_nonzero == 0 else RHS_OUT_OF_RANGE


def classify_rhs(b, bnorm2, target):
    """classify_rhs (krylov.hip) with count_entries_kernel (blas1.hip): the verdict, and None or the Result that ends the solve"""
    b = np.asarray(b, np.float64)
    v = rhs_verdict(bnorm2, target, int((~np.isfinite(b)).sum()), int((b != 0.0).sum()))
    if v == RHS_ORDINARY:
        return v, None
    if v == RHS_ZERO:
        return v, Result(np.zeros(b.size), 0, OK, 0.0, [], False, 1.0)
    return v, Result(np.full(b.size, np.nan), 0, BREAKDOWN, math.nan, [], False, 1.0)


def _fmax(a, b):
    """fmax of C: a NaN operand is ignored"""
    return b if a != a else a if b != b else max(a, b)


def _sqrt(v):
    """sqrt of a sum of squares as C takes it: NaN stays NaN (math.sqrt raises on nothing a sum of squares can be)"""
    return math.sqrt(v) if v == v else math.nan


def berr(r, den):
    """berr_kernel / max_partials_kernel (blas1.hip): max_i |r_i| / den_i, a row with den_i = 0 counting 1e300 when r_i != 0 and
    nothing when r_i = 0 -- and NaN as soon as any quotient is (a NaN in r or den, Inf / Inf)"""
    a, d = np.abs(np.asarray(r, np.float64)), np.asarray(den, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where((d > 0.0) | np.isnan(d), a / d, np.where(np.isnan(a), a, np.where(a > 0.0, 1.0e300, 0.0)))
    if np.isnan(q).any():
        return math.nan
    return float(q.max()) if q.size else 0.0


def _dist(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0.0 else 0.0


def chained_precond(A, M, steps):
    """apply_precond (krylov.hip): z = M r, then z += M (r - A z) for every further cycle"""
    def apply(r):
        z = M(r)
        for _ in range(1, steps):
            z = z + M(r - A(z))
        return z
    return apply


def row_equilibration(rowptr, val):
    """upload_row_scales (create.hip): R_i = 1 / max_j |a_ij| and its inverse max_j |a_ij|; rows without entries keep 1"""
    rowptr = np.asarray(rowptr, np.int64)
    n = rowptr.size - 1
    mx = np.zeros(n)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    np.maximum.at(mx, rows, np.abs(np.asarray(val, np.float64)))
    rs, ri = np.ones(n), np.ones(n)
    rs[mx > 0.0] = 1.0 / mx[mx > 0.0]
    ri[mx > 0.0] = mx[mx > 0.0]
    return rs, ri


def fgmres(A, M, b, x0=None, *, restart, max_iters, rtol=1e-10, atol=0.0, reorth=0, basis_f32=0, rscale=None, rinv=None,
           precond_steps=1, pythagoras=False, arith=None, trace=None):
    """Restarted right-preconditioned flexible GMRES as csrc/krylov.hip runs it.  rscale (with rinv = its inverse as the library
    stores it, default 1 / rscale) turns the iteration into the row-weighted one on R A M R^-1.  pythagoras is the epilogue
    of a row-distributed solver with one reduction per step (it replaces the plain norm; with reorth it is not used)."""
    ar = arith or Arith()
    b = np.asarray(b, np.float64)
    n, m = b.size, int(restart)
    log = []

    def decide(kind, its, lhs, rhs, taken):
        log.append(Decision(kind, its, lhs, rhs, bool(taken), _dist(lhs, rhs)))
        return taken

    def note(*event):
        if trace is not None:
            trace.append(event)

    # ---- fg_begin (krylov.hip)
    bnorm2 = ar.dot(b, b)
    bnorm = _sqrt(bnorm2)
    target = _fmax(rtol * bnorm, atol)
    _, over = classify_rhs(b, bnorm2, target)
    if over is not None:
        return over
    steps_now = precond_steps
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64)
    if rscale is not None and rinv is None:
        rinv = 1.0 / rscale
    H = np.zeros((m, m + 1))                      # H[j] = column j, as F.H[j * (m + 1) + i]
    cs, sn, g, y = np.zeros(m), np.zeros(m), np.zeros(m + 1), np.zeros(m)
    its, status, relres, stagnated = 0, NOT_CONVERGED, 0.0, False
    stalled_cycles, inner_scale, beta_prev, est_at_exit, ended_on_estimate = 0, 1.0, 0.0, 0.0, False

    while True:
        # ---- fg_restart (krylov.hip; the verdict: krylov_host.cpp, fg_restart_verdict)
        r = b - A(x)
        beta = _sqrt(ar.dot(r, r))
        relres = beta / bnorm
        note("restart", beta)
        if not math.isfinite(beta):
            status, relres = BREAKDOWN, math.nan
            break
        if decide("converged", its, beta, target, beta <= target):
            status = OK
            break
        if its >= max_iters:
            status = NOT_CONVERGED
            break
        if steps_now > 1 and its > 0 and decide("demote", its, beta, beta_prev, not beta < beta_prev):
            steps_now = 1
        if ended_on_estimate and decide("stall", its, beta, 0.7 * beta_prev, beta > 0.7 * beta_prev):
            stalled_cycles += 1
        else:
            stalled_cycles = 0
        if stalled_cycles >= 3:
            status, stagnated = NOT_CONVERGED, True
            break
        if ended_on_estimate and est_at_exit > 0.0:
            inner_scale = max(1e-3, min(inner_scale, 0.5 * est_at_exit / beta))
        beta_prev = beta
        ended_on_estimate = False
        note("cycle", steps_now, stalled_cycles, inner_scale)
        beta_it, target_it = beta, target
        if rscale is not None:
            r = r * rscale
            beta_it = math.sqrt(ar.dot(r, r))
            if not beta_it > 0.0:
                status = BREAKDOWN
                break
            target_it = target * (beta_it / beta)
        vcur, vf = ar.scale_to(r, 1.0 / beta_it, basis_f32)
        V = [vf if basis_f32 else vcur]           # the Gram-Schmidt operands: the f32 copies with basis_f32
        Z = []
        g[0] = beta_it
        j = 0
        breakdown_in_cycle = False
        precond = chained_precond(A, M, steps_now)

        while True:
            # ---- arnoldi_apply (krylov.hip): M sees the f64 twin of the newest basis vector
            vj = vcur
            if rscale is not None:
                z = precond(vj * rinv)
                w = A(z) * rscale
            else:
                z = precond(vj)
                w = A(z)
            Z.append(z)
            # ---- arnoldi_orthogonalise (krylov.hip)
            h = np.array([ar.dot(V[i], w) for i in range(j + 1)] + [ar.dot(w, w)])
            w = ar.update(w, V, h)
            nrm2 = ar.dot(w, w)
            if reorth:
                h2 = np.array([ar.dot(V[i], w) for i in range(j + 1)])
                w = ar.update(w, V, h2)
                nrm2 = ar.dot(w, w)
                h[:j + 1] += h2                   # finish_column_body (blas1.hip:419-429)
                t = math.sqrt(nrm2)
                h[j + 1] = t
            elif pythagoras:
                # finish_column_pythagoras_body (blas1.hip:442-456)
                ww = h[j + 1]
                t2 = ww - ar.sumsq(h[:j + 1])
                weak = decide("weak", its, t2, 1e-8 * ww, not t2 >= 1e-8 * ww)
                if not t2 > 0.0:
                    t2 = 0.0
                t = math.sqrt(t2)
                h[j + 1] = -t if weak else t
            else:
                t = math.sqrt(nrm2)
                h[j + 1] = t
            vcur, vf = ar.scale_to(w, 1.0 / t if t > 0.0 else 0.0, basis_f32)
            V.append(vf if basis_f32 else vcur)

            # ---- fg_post_step (krylov.hip; krylov_host.cpp, fg_column_step)
            hc = H[j]
            hc[:j + 2] = h
            weak_norm = hc[j + 1] < 0.0
            if weak_norm:
                hc[j + 1] = -hc[j + 1]
            for i in range(j):
                tt = cs[i] * hc[i] + sn[i] * hc[i + 1]
                hc[i + 1] = -sn[i] * hc[i] + cs[i] * hc[i + 1]
                hc[i] = tt
            hjj, hj1 = hc[j], hc[j + 1]
            d = math.hypot(hjj, hj1)
            if not d > 0.0 or d != d:
                status, breakdown_in_cycle = BREAKDOWN, True          # column j is unusable: keep k = j
                note("step", h.copy(), its, None, True)
                break
            cs[j], sn[j] = hjj / d, hj1 / d
            hc[j], hc[j + 1] = d, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            its += 1
            est = abs(g[j + 1])
            j += 1
            if decide("estimate", its, est, target_it * inner_scale, est <= target_it * inner_scale) or hj1 == 0.0:
                ended_on_estimate = True
                est_at_exit = est * (beta / beta_it)
                note("step", h.copy(), its, est, True)
                break
            ends = weak_norm or j >= m or its >= max_iters
            note("step", h.copy(), its, est, ends)
            if ends:
                break

        # ---- fg_end_cycle (krylov.hip; krylov_host.cpp, fg_back_substitute)
        k = j
        for i in range(k - 1, -1, -1):
            tt = g[i]
            for c in range(i + 1, k):
                tt -= H[c][i] * y[c]
            y[i] = tt / H[i][i]
        note("end", k, y[:k].copy(), cs[:k].copy(), sn[:k].copy(), g[:k + 1].copy(), [H[c][:c + 1].copy() for c in range(k)])
        x = ar.update(x, Z[:k], y, sign=1.0)
        if breakdown_in_cycle:
            r = b - A(x)
            rn = _sqrt(ar.dot(r, r))
            relres = rn / bnorm if math.isfinite(rn) else math.nan
            status = OK if rn <= target else BREAKDOWN
            break
    return Result(x, its, status, relres, log, stagnated, inner_scale)


def bicgstab(A, M, b, x0=None, *, max_iters, rtol=1e-10, atol=0.0, precond_steps=1, arith=None):
    """Right-preconditioned BiCGStab (krylov.hip, bicgstab), the 1.0001 slack on the final true residual included."""
    ar = arith or Arith()
    b = np.asarray(b, np.float64)
    n = b.size
    log = []

    def decide(kind, its, lhs, rhs, taken):
        log.append(Decision(kind, its, lhs, rhs, bool(taken), _dist(lhs, rhs)))
        return taken

    precond = chained_precond(A, M, precond_steps)
    rho = alpha = omega = 1.0
    bnorm2 = ar.dot(b, b)
    bnorm = _sqrt(bnorm2)
    target = _fmax(rtol * bnorm, atol)
    _, over = classify_rhs(b, bnorm2, target)
    if over is not None:
        return over
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64)
    r = b - A(x)
    r0 = r.copy()
    p, v = np.zeros(n), np.zeros(n)
    its, status = 0, NOT_CONVERGED
    rn2 = ar.dot(r, r)
    while its < max_iters:
        if not math.isfinite(rn2):
            status = BREAKDOWN
            break
        if decide("converged", its, math.sqrt(rn2), target, math.sqrt(rn2) <= target):
            status = OK
            break
        rho_new = ar.dot(r0, r)
        if rho_new == 0.0 or rho_new != rho_new:
            status = BREAKDOWN
            break
        beta = (rho_new / rho) * (alpha / omega)
        p = 1.0 * p + (-omega) * v               # axpby_kernel (blas1.hip:297-308): y = b y + a x
        p = beta * p + 1.0 * r
        ph = precond(p)
        v = A(ph)
        tmp = ar.dot(r0, v)
        if tmp == 0.0 or tmp != tmp:
            status = BREAKDOWN
            break
        alpha = rho_new / tmp
        sv = 1.0 * r + (-alpha) * v
        sh = precond(sv)
        t = A(sh)
        ts, tt = ar.dot(t, sv), ar.dot(t, t)
        if tt == 0.0 or tt != tt:
            status = BREAKDOWN
            break
        omega = ts / tt
        x = 1.0 * x + alpha * ph
        x = 1.0 * x + omega * sh
        r = 1.0 * sv + (-omega) * t
        rho = rho_new
        its += 1
        rn2 = ar.dot(r, r)
        if omega == 0.0:
            status = BREAKDOWN
            break
    r = b - A(x)
    rn = _sqrt(ar.dot(r, r))
    relres = rn / bnorm
    if not math.isfinite(rn):
        status, relres = BREAKDOWN, math.nan
    elif decide("final", its, rn, target * 1.0001, rn <= target * 1.0001):
        status = OK
    elif status == OK:
        status = NOT_CONVERGED
    return Result(x, its, status, relres, log, False, 1.0)
