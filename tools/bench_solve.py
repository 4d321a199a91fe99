"""One GPU, one handle: what a block of right-hand sides costs beside single pangulu_gstrs calls on the same factors.

    python tools/bench_solve.py [--matrix elastic3d] [--size 48] [--nb 256] [--vtype r64] [--nrhs 1,4,16,64] [--repeats 5] [--trans N|T|H] [--device-rhs] [--rcond]

After pangulu_gstrf it times, in this process, the median of `repeats` single pangulu_gstrs calls and the median of `repeats`
pangulu_gstrs_multi calls per nrhs, and prints one JSON line: the times, the time per column, the panels, the factor bytes a panel
streams (info.owned_bytes: every record is read once per panel) and the bandwidth that implies.  The yardstick is nrhs single
calls.  --trans T|H also times the transposed solves (A^T X = B, A^H X = B) of the same handle, the single call and every nrhs, beside
their untransposed twins: a transposed sweep streams the same factor bytes, so the untransposed time of the same run is its yardstick
(matrices here are symmetric or nearly so: the residual is that of the transposed system all the same).  --device-rhs also times pangulu_amd_gstrs_device
on a column-major device buffer beside pangulu_amd_gstrs_multi / _trans on a host buffer of the same handle, the raw C calls in place, per nrhs
(and for --trans): both return synchronised, so a host perf_counter around the call is the time; the host-pointer call is the yardstick and
its own spread (min .. max of the repeats) the margin.  --rcond times pangulu_amd_rcond (1-norm) and prints its number of solves and its
milliseconds beside `solves` x the time of one single-column pangulu_amd_gstrs_device solve of the same run (the mean of the A and the A^H
solve: the estimator alternates between them), so that what the vector kernels and the read-backs between the solves cost is visible.  (Run it through `tools/gpu_job.sh solve`, which puts it under a time limit.)"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pangulu_amd as pa  # noqa: E402
from pangulu_amd import _lib, matrices as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", default="elastic3d", choices=["elastic3d", "fem27", "poisson3d", "shell", "kkt"])
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--vtype", default="r64", choices=sorted(_lib.VALUE_TYPES))
    ap.add_argument("--nrhs", default="1,4,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trans", default="N", choices=["N", "T", "H"])
    ap.add_argument("--device-rhs", action="store_true")
    ap.add_argument("--rcond", action="store_true")
    a = ap.parse_args()
    if a.device_rhs or a.rcond:
        # torch brings a HIP runtime of its own under the same soname as the one the library links: a process gets whichever is loaded
        # first, and torch finds no device on the other one.  So torch first -- as in bench.py and the tests -- and both calls on it.
        import torch

        torch.cuda.init()
    dt = _lib.VALUE_TYPES[a.vtype][0]
    cplx = np.issubdtype(dt, np.complexfloating)
    if a.matrix == "poisson3d":
        mat = M.poisson3d(a.size, dtype=dt, shift=0.5j if cplx else 0.0)
    elif a.matrix == "shell":
        mat = M.shell(a.size, a.size, dtype=dt)
    else:
        mat = getattr(M, a.matrix)(a.size, dtype=dt)
    n, cp, ri, va, co = mat
    lib = _lib.load(a.vtype)
    lib.pangulu_amd_reset_options()
    h = pa.pangulu_init(n, len(va), cp, ri, va, nb=a.nb, vtype=a.vtype, coords=co, nthread=16)
    t0 = time.time()
    pa.pangulu_gstrf(h)
    t_gstrf = time.time() - t0
    info = h.info()
    widths = [int(w) for w in a.nrhs.split(",")]
    rng = np.random.default_rng(7)
    B = rng.uniform(-1.0, 1.0, size=(n, max(widths))).astype(dt)
    B[:, 0] = M.rhs_of_ones(n, cp, ri, va)

    def median_of(f):
        f()  # (warm-up: first-use allocations, the cached sweep plan)
        ts = []
        for _ in range(a.repeats):
            t = time.time()
            f()
            ts.append(time.time() - t)
        return statistics.median(ts)

    def spread_of(f):
        f()
        ts = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t)
        return {"median_s": round(statistics.median(ts), 6), "min_s": round(min(ts), 6), "max_s": round(max(ts), 6)}

    def device_beside_host(Bw, trans):
        """the raw calls, each in place on a buffer of its own (what a buffer holds does not change what a sweep costs)"""
        import torch

        w, code, opt = Bw.shape[1], {"N": 0, "T": 1, "H": 2}[trans], _lib.GstrsOptions()
        hbuf = np.array(Bw, order="F", copy=True)
        dbuf = torch.from_numpy(np.ascontiguousarray(Bw.T)).cuda().t()  # (n, w), column-major
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        hptr, dptr = hbuf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dbuf.data_ptr())

        def host_call():
            assert lib.pangulu_amd_gstrs_trans(hptr, w, n, code, ctypes.byref(opt), h.ref) == 0

        def device_call():
            assert lib.pangulu_amd_gstrs_device(dptr, w, n, code, stream, ctypes.byref(opt), h.ref) == 0

        hbuf[:] = Bw
        host_call()
        Xh = hbuf.copy()
        device_call()
        torch.cuda.synchronize()
        Xd = dbuf.cpu().numpy()
        path = pa.last_solve_path(h)
        th, td = spread_of(host_call), spread_of(device_call)
        return {"trans": trans, "host_pointer": th, "device_pointer": td, "device_vs_host": round(td["median_s"] / th["median_s"], 3),
                "device_columns": path["device_columns"], "panels": path["panels"],
                "first_solve_difference": float("%.2e" % (np.abs(Xd - Xh).max() / np.abs(Xh).max()))}

    b0 = np.ascontiguousarray(B[:, 0])
    x_single = pa.pangulu_gstrs(h, b0)
    t_single = median_of(lambda: pa.pangulu_gstrs(h, b0))
    out = {"tool": "bench_solve", "matrix": "%s(%d)" % (a.matrix, a.size), "vtype": a.vtype, "n": n, "nb": a.nb, "gstrf_s": round(t_gstrf, 4),
           "owned_bytes": int(info["owned_bytes"]), "gstrs_single_s": round(t_single, 5),
           "gstrs_single_gbs": round(info["owned_bytes"] / t_single / 1e9, 1), "multi": []}
    if a.trans != "N":
        At = M.to_scipy(n, cp, ri, va).T.tocsc()
        if a.trans == "H":
            At = At.conj()

        def trans_residual(x, b):
            return float(np.linalg.norm(At @ x - b) / np.linalg.norm(b))

        pa.pangulu_gstrs(h, b0, trans=a.trans)
        t_single_t = median_of(lambda: pa.pangulu_gstrs(h, b0, trans=a.trans))
        out.update({"trans": a.trans, "trans_single_s": round(t_single_t, 5), "trans_single_gbs": round(info["owned_bytes"] / t_single_t / 1e9, 1),
                    "trans_single_vs_untransposed": round(t_single_t / t_single, 3)})
    for w in widths:
        Bw = np.asfortranarray(B[:, :w])
        X = pa.pangulu_gstrs_multi(h, Bw)
        path = pa.last_solve_path(h)
        t = median_of(lambda: pa.pangulu_gstrs_multi(h, Bw))
        res = max(M.relative_residual(n, cp, ri, va, X[:, j], Bw[:, j]) for j in range(w))
        out["multi"].append({"nrhs": w, "seconds": round(t, 5), "seconds_per_column": round(t / w, 6), "speedup_vs_single_calls": round(t_single * w / t, 2),
                             "device_columns": path["device_columns"], "panel_width": path["panel_width"], "panels": path["panels"],
                             "factor_bytes_per_panel": int(info["owned_bytes"]), "implied_gbs": round(path["panels"] * info["owned_bytes"] / t / 1e9, 1),
                             "worst_residual": float("%.2e" % res),
                             "column0_vs_single": float("%.2e" % (np.abs(X[:, 0] - x_single).max() / np.abs(x_single).max()))})
        if a.trans != "N":
            Xt = pa.pangulu_gstrs_multi(h, Bw, trans=a.trans)
            pt = pa.last_solve_path(h)
            tt = median_of(lambda: pa.pangulu_gstrs_multi(h, Bw, trans=a.trans))
            out["multi"][-1]["trans"] = {"seconds": round(tt, 5), "vs_untransposed": round(tt / t, 3), "device_columns": pt["device_columns"],
                                         "panel_width": pt["panel_width"], "panels": pt["panels"],
                                         "implied_gbs": round(pt["panels"] * info["owned_bytes"] / tt / 1e9, 1),
                                         "worst_residual": float("%.2e" % max(trans_residual(Xt[:, j], Bw[:, j]) for j in range(w)))}
        if a.device_rhs:
            out["multi"][-1]["device_rhs"] = [device_beside_host(Bw, t) for t in (["N"] if a.trans == "N" else ["N", a.trans])]
    if a.rcond:
        import torch

        opt = _lib.GstrsOptions()
        dcol = torch.from_numpy(np.ascontiguousarray(B[:, 0])).cuda()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        one_column = {}
        for name, code in (("N", 0), ("H", 2)):
            rc = lib.pangulu_amd_gstrs_device(ctypes.c_void_p(dcol.data_ptr()), 1, n, code, stream, ctypes.byref(opt), h.ref)
            if rc == 0:  # (4: no device-resident path for this handle; the estimator then runs on the host as well)
                one_column[name] = spread_of(lambda: lib.pangulu_amd_gstrs_device(ctypes.c_void_p(dcol.data_ptr()), 1, n, code, stream, ctypes.byref(opt), h.ref))
        d = pa.rcond(h, "1", details=True)
        t = spread_of(lambda: pa.rcond(h, "1"))
        out["rcond"] = dict(d, norm="1", call_ms=round(1e3 * t["median_s"], 3), call_min_ms=round(1e3 * t["min_s"], 3), call_max_ms=round(1e3 * t["max_s"], 3))
        if len(one_column) == 2:
            single = 0.5 * (one_column["N"]["median_s"] + one_column["H"]["median_s"])
            out["rcond"].update({"device_rhs_single_column_ms": {k: round(1e3 * v["median_s"], 3) for k, v in one_column.items()},
                                 "solves_x_single_column_ms": round(1e3 * d["solves"] * single, 3),
                                 "call_vs_solves": round(t["median_s"] / (d["solves"] * single), 3)})
        print("rcond_1 = %.6e: %d solves, %.3f ms (solves x one device-rhs single-column solve: %s ms)"
              % (d["rcond"], d["solves"], out["rcond"]["call_ms"], out["rcond"].get("solves_x_single_column_ms", "n/a")), flush=True)
    pa.pangulu_finalize(h)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
