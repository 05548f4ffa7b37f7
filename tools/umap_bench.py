#!/usr/bin/env python3
"""UMAP of synthetic latents on the MI355X (UMAPHIP, vame_amd/analysis/umap_hip.py): one JSON line with the time of each stage at the
reference's default shape (num_points 30000, n_neighbors 200, 30 latent dimensions, 200 epochs) on 10-blob latents.

    python tools/umap_bench.py [N] [--sklearn]

Stage times are host clocks around work that ends in a device synchronise, after one warm-up fit of the same shape.  The kNN kernel
is also timed alone with device events; its rate counts 2 N^2 D operations (a subtraction and an FMA per dimension and pair) against the
157.3 TFLOP/s fp32 vector peak.  --sklearn adds sklearn NearestNeighbors(algorithm="brute") on the host as the CPU figure for the kNN
step.  There is no end-to-end CPU baseline: umap-learn is not installed.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vame_amd.analysis.umap_hip import UMAPHIP, default_epochs  # noqa: E402

FP32_VALU_PEAK = 157.3e12
args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 30000
D, K, n_blobs = 30, 200, 10
rng = np.random.default_rng(0)
cent = rng.standard_normal((n_blobs, D)) * 4
X = (cent[rng.integers(0, n_blobs, N)] + rng.standard_normal((N, D))).astype(np.float32)
n_epochs = default_epochs(N)


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def stages(um, Xd):
    t = {}
    t0 = sync()
    idx, dist = um.knn(Xd, K)
    t1 = sync()
    _, _, w = um.membership(idx, dist)
    t2 = sync()
    um._graph = None
    um._csr = um.graph(idx, w, n_epochs)
    t3 = sync()
    Y0 = um.initial(N, 42)
    t4 = sync()
    um.layout(Y0, *um._csr, n_epochs, 42)
    t5 = sync()
    t.update(knn_ms=(t1 - t0) * 1e3, membership_ms=(t2 - t1) * 1e3, graph_ms=(t3 - t2) * 1e3, init_host_ms=(t4 - t3) * 1e3,
             epochs_ms=(t5 - t4) * 1e3, total_ms=(t5 - t0) * 1e3)
    return t, idx


Xd = torch.from_numpy(X).cuda()
um = UMAPHIP(n_neighbors=K, min_dist=0.1, random_state=42)
stages(um, Xd)                                                   # warm-up: code objects, allocator, the a / b fit
t, idx = stages(um, Xd)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
reps = 5
e0.record()
for _ in range(reps):
    um.knn(Xd, K)
e1.record()
torch.cuda.synchronize()
knn_kernel_ms = e0.elapsed_time(e1) / reps
ops_knn = 2.0 * N * N * D
out = dict(N=N, D=D, k=K, n_epochs=n_epochs, init=um.init_used_, edges=int(um._csr[1].numel()),
           **{k: round(v, 3) for k, v in t.items()},
           epoch_ms=round(t["epochs_ms"] / n_epochs, 4), knn_kernel_ms=round(knn_kernel_ms, 3),
           knn_tflops=round(ops_knn / knn_kernel_ms / 1e9, 2), knn_frac_fp32_valu_peak=round(ops_knn / knn_kernel_ms / 1e9 / (FP32_VALU_PEAK / 1e12), 3),
           cpu_end_to_end="none: umap-learn is not installed, so there is no CPU UMAP to compare with")
if "--sklearn" in sys.argv:
    from sklearn.neighbors import NearestNeighbors
    t0 = time.perf_counter()
    NearestNeighbors(n_neighbors=K, algorithm="brute").fit(X).kneighbors(X)
    out.update(sklearn_brute_knn_ms=round((time.perf_counter() - t0) * 1e3, 1), host_threads=len(os.sched_getaffinity(0)))
print(json.dumps(out))
