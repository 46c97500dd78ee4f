"""The transport's callbacks, wrapped so that the distributed workers can record the order of the collective calls a library call
makes (a plain helper module, imported by the dist_*_worker.py scripts)."""
import ctypes as C

AGREE = "allgather_i64_host"
# an operand call on a row-distributed solver (nkp_value_gradient*, nkp_values_product*, the steady state of
# nkp_values_product_trans_dist*): the first agreement, ONE exchange, the second agreement; a rank with a bad argument makes every
# rank leave after the first agreement
GOOD_CALL = [AGREE, "alltoallv", AGREE]
REFUSED_CALL = [AGREE]


def traced(solver, ops, log):
    """a copy of ops whose four callbacks append their name (and the reduction's count and op) to log and call the transport's"""
    orig = solver.NkpCommOps()
    C.memmove(C.byref(orig), C.byref(ops), C.sizeof(solver.NkpCommOps))

    def allreduce(ctx, buf, count, op, st):
        log.append(f"allreduce {'max' if op else 'sum'} {count}")
        return orig.allreduce(ctx, buf, count, op, st)

    def alltoallv(ctx, send, sc, recv, rc, st):
        log.append("alltoallv")
        return orig.alltoallv(ctx, send, sc, recv, rc, st)

    def alltoallv_i32(ctx, send, sc, recv, rc):
        log.append("alltoallv_i32_host")
        return orig.alltoallv_i32_host(ctx, send, sc, recv, rc)

    def allgather(ctx, mine, out):
        log.append("allgather_i64_host")
        return orig.allgather_i64_host(ctx, mine, out)

    w = solver.NkpCommOps()
    w.ctx, w.rank, w.nranks = ops.ctx, ops.rank, ops.nranks
    w.allreduce = solver._ALLREDUCE_FN(allreduce)
    w.alltoallv = solver._ALLTOALLV_FN(alltoallv)
    w.alltoallv_i32_host = solver._ALLTOALLV_I32_FN(alltoallv_i32)
    w.allgather_i64_host = solver._ALLGATHER_I64_FN(allgather)
    return w, orig


class Recorder:
    """the trace (log is the list the traced callbacks append to) and the deltas of the solver's counters over one call"""

    def __init__(self, log, calls_key):
        self.log, self.calls_key = log, calls_key

    def counters(self, s):
        return dict(alltoallv=s.get_int("dist_alltoallv_calls"), allreduce=s.get_int("dist_allreduce_calls"), calls=s.get_int(self.calls_key))

    def run(self, s, fn):
        """(trace, counter deltas, what fn returned) of fn () on solver s"""
        c0 = self.counters(s)
        del self.log[:]
        out = fn()
        trace = list(self.log)
        c1 = self.counters(s)
        return dict(trace=trace, counters={k: c1[k] - c0[k] for k in c0}), out
