"""One GPU, one handle: what new values on a fixed pattern cost from a numpy array and from a CUDA tensor.

    python tools/bench_update_values.py [--matrix elastic3d] [--size 48] [--nb 256] [--vtype r64] [--repeats 5]

After pangulu_init and one pangulu_gstrf it alternates, in this process, pa.update_values from a numpy array (pangulu_amd_update_values:
every record refilled on the host, the whole arena uploaded -- the yardstick) and pa.update_values from a CUDA tensor
(pangulu_amd_update_values_device: two kernels over a map kept on the device, nnz values to the host), a pangulu_gstrf after each so
that every call finds factors in the records as a Newton iteration would leave them.  Both calls return synchronised, so a host
perf_counter around the call is its time.  The first device call builds the map and is reported on its own; then one warm-up pair
and `repeats` timed pairs.  Prints one JSON line: medians, minima and maxima, the ratio host median / device median, whether the
device median lies below the host minimum, the bytes each path moves over the host link (host: the arena up, info.owned_bytes;
device: nnz values down) and the device bytes the map holds.  The records after the last device call are compared bit for bit with
those after the last host call (same values).  (Run it through `tools/gpu_job.sh values`, which puts it under a time limit.)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime per process, see tools/bench_solve.py)

import pangulu_amd as pa  # noqa: E402
from pangulu_amd import _lib, matrices as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", default="elastic3d", choices=["elastic3d", "fem27", "poisson3d", "shell"])
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--vtype", default="r64", choices=sorted(_lib.VALUE_TYPES))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()
    dt = _lib.VALUE_TYPES[a.vtype][0]
    mat = M.shell(a.size, a.size, dtype=dt) if a.matrix == "shell" else getattr(M, a.matrix)(a.size, dtype=dt)
    n, cp, ri, va, co = mat
    lib = _lib.load(a.vtype)
    lib.pangulu_amd_reset_options()
    h = pa.pangulu_init(n, len(va), cp, ri, va, nb=a.nb, vtype=a.vtype, coords=co, nthread=16)
    info = h.info()
    rng = np.random.default_rng(11)
    # same pattern, other values, the diagonal untouched (diagonally dominant matrices stay so)
    scale = rng.uniform(0.9, 1.0, len(va))
    rows = np.asarray(ri, dtype=np.int64)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(cp, dtype=np.int64)))
    scale[rows == cols] = 1.0
    new = np.ascontiguousarray(va * scale, dtype=dt)
    d_new = torch.from_numpy(new).cuda()
    torch.cuda.synchronize()

    def timed(values):
        t = time.perf_counter()
        pa.update_values(h, values)
        return time.perf_counter() - t

    def gstrf():
        t = time.perf_counter()
        pa.pangulu_gstrf(h)
        return time.perf_counter() - t

    t_gstrf = [gstrf()]
    first_device = timed(d_new)  # (builds and uploads the map)
    t_gstrf.append(gstrf())
    host, device = [], []
    for k in range(a.repeats + 1):  # (pair 0: warm-up)
        th = timed(new)
        t_gstrf.append(gstrf())
        td = timed(d_new)
        if k < a.repeats:
            t_gstrf.append(gstrf())
        if k > 0:
            host.append(th)
            device.append(td)
    after_device = [v.copy() for *_, v in pa.owned_blocks(h)]
    pa.update_values(h, new)
    same = all(x.tobytes() == y.tobytes() for x, (*_, y) in zip(after_device, pa.owned_blocks(h)))
    pa.pangulu_gstrf(h)
    check, replayed = pa.factor_check(h), int(h.info()["replayed"])
    map_bytes = pa.hip_memory(h)["values_refresh_bytes"]
    pa.pangulu_finalize(h)

    def spread(ts):
        return {"median_s": round(statistics.median(ts), 6), "min_s": round(min(ts), 6), "max_s": round(max(ts), 6)}

    out = {"tool": "bench_update_values", "matrix": "%s(%d)" % (a.matrix, a.size), "nb": a.nb, "vtype": a.vtype, "n": n, "nnz": len(va),
           "repeats": a.repeats, "host_numpy": spread(host), "device_tensor": spread(device), "first_device_call_s": round(first_device, 6),
           "host_median_over_device_median": round(statistics.median(host) / statistics.median(device), 2),
           "device_median_below_host_min": bool(statistics.median(device) < min(host)),
           "host_link_bytes": {"host_numpy": int(info["owned_bytes"]), "device_tensor": int(len(va) * np.dtype(dt).itemsize)},
           "map_device_bytes": int(map_bytes), "records_bit_equal": bool(same), "gstrf_median_s": round(statistics.median(t_gstrf), 6),
           "factor_check": check, "replayed": replayed}
    print(json.dumps(out))
    return 0 if same and out["device_median_below_host_min"] else 1


if __name__ == "__main__":
    sys.exit(main())
