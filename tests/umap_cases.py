"""Shared UMAP test bodies (vame_amd/csrc/umap.hip, vame_amd/analysis/umap_hip.py, vame.visualization): run on `cpu` tensors through
the emulator or on `cuda` through libvame_hip.so.  The numpy restatements below follow the rules as include/vame_hip.h states them;
umap-learn is not installed and nothing here comes from it."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from kernel_cases import N_, T_, philox4x32_10
from vame_amd import ops

f32 = np.float32


# ------------------------------------------------------------------ restatements
def knn_ref64(X, rows=None):
    """float64 distances of `rows` (default all) to every point; the row's own point first, then the others by (distance, index)."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    rows = np.arange(N) if rows is None else np.asarray(rows)
    orders, dists = [], []
    step = max(1, int(2e7 // (N * D)))                        # blocks of rows: ~160 MB of float64 differences at a time
    for r0 in range(0, len(rows), step):
        rr = rows[r0:r0 + step]
        d = np.sqrt(((X[rr, None, :] - X[None, :, :]) ** 2).sum(-1))
        d[np.arange(len(rr)), rr] = -1.0                      # self first
        order = np.lexsort((np.broadcast_to(np.arange(N), d.shape), d), axis=1)
        d[np.arange(len(rr)), rr] = 0.0
        orders.append(order)
        dists.append(np.take_along_axis(d, order, 1))
    return np.concatenate(orders), np.concatenate(dists)


def check_knn_rows(X, idx, dist, rows, k):
    """idx / dist rows `rows` of the kernel against float64: slot 0, neighbour sets up to near-ties at the k-th place, distances."""
    order, dref = knn_ref64(X, rows)
    X64 = np.asarray(X, dtype=np.float64)
    for n, i in enumerate(rows):
        assert idx[i, 0] == i and dist[i, 0] == 0.0, (i, idx[i, :3], dist[i, :3])
        assert np.all(np.diff(dist[i]) >= 0), i
        got = idx[i, 1:]
        assert len(set(got.tolist())) == k - 1 and i not in set(got.tolist())
        if set(got.tolist()) != set(order[n, 1:k].tolist()):
            gap = dref[n, k] - dref[n, k - 1] if k < X.shape[0] else np.inf
            assert gap <= 1e-6 * dref[n, k - 1], (i, gap)
        dtrue = np.sqrt(((X64[got] - X64[i]) ** 2).sum(-1))
        np.testing.assert_allclose(dist[i, 1:], dtrue, rtol=1e-6, atol=1e-30)


def membership_ref(dist, idx):
    """rho, sigma (float64), w (N, k) and whether the bisection converged, per row."""
    N, k = dist.shape
    d = dist.astype(np.float64)
    mean_all = d.mean()
    target = np.log2(k)
    rho, sigma, conv = np.zeros(N), np.zeros(N), np.zeros(N, bool)
    w = np.zeros((N, k))
    for i in range(N):
        row = d[i]
        nz = row[row > 0]
        r = nz.min() if nz.size else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            dd = row[1:] - r
            ps = np.where(dd > 0, np.exp(-np.maximum(dd, 0.0) / mid), 1.0).sum()
            if abs(ps - target) < 1e-5:
                conv[i] = True
                break
            if ps > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if hi == np.inf else (lo + hi) / 2
        floor_ = 1e-3 * (row.mean() if r > 0 else mean_all)
        if mid < floor_:
            mid = floor_
            conv[i] = False
        rho[i], sigma[i] = r, mid
        dd = row - r
        w[i] = np.where((dd <= 0) | (mid == 0), 1.0, np.exp(-np.maximum(dd, 0.0) / mid))
        w[i, idx[i] == i] = 0.0
    return rho, sigma, w, conv


def graph_ref(idx, w, n_epochs):
    """scipy restatement of the pruned fuzzy union, float32 like the kernels."""
    N, k = idx.shape
    rows, cols, vals = np.repeat(np.arange(N), k), idx.ravel().astype(np.int64), np.asarray(w, dtype=f32).ravel()
    m = cols != rows
    W = sp.csr_matrix((vals[m], (rows[m], cols[m])), shape=(N, N), dtype=f32)
    P = (W + W.T - W.multiply(W.T)).tocsr()
    P.eliminate_zeros()
    thr = f32(P.data.max()) / f32(n_epochs)
    P.data[P.data < thr] = 0
    P.eliminate_zeros()
    P.sort_indices()
    return P


def _libm_powf():
    """powf of the C library: the emulator build's kernels call it, so the restatement does too (numpy's float32 power rounds
    differently in the last place for ~20 % of arguments)"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    fn = libm.powf
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    return lambda x, y: f32(fn(float(x), float(y)))


_powf = _libm_powf()


def assert_layout_close(got, ref, what, exact=True):
    """Layouts of the same rule.  exact (the emulator: the same libm as the restatement): every coordinate to 1e-5.  Otherwise (the
    device's own powf, which differs from the C library's in the last place): the SGD map amplifies a last-place difference where a
    negative sample lands within ~1e-3 of the vertex (the repulsion gradient there is ~2b / 0.001), and once the early epochs have
    pulled neighbours together that happens for a few vertices per epoch (measured: 98 % of the coordinates within 1e-5 in the second
    epoch of check_pipeline, the rest within 7e-3).  95 % must agree to 1e-5."""
    close = np.isclose(got, ref, rtol=1e-5, atol=1e-5)
    if exact:
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5, err_msg=what)
    else:
        assert close.mean() >= 0.95 and np.isfinite(got).all(), (what, close.mean(), np.abs(got - ref).max())


def _fma32(x, y, z):
    return f32(float(x) * float(y) + float(z))


def _clip4(v):
    return f32(min(max(v, f32(-4)), f32(4)))


def epoch_ref(Y, indptr, indices, rate, epoch, alpha, a, b, seed):
    """One epoch of vame_umap_epoch_f32 in float32 scalar arithmetic (the rule of include/vame_hip.h)."""
    N = Y.shape[0]
    Yin = np.asarray(Y, dtype=f32)
    Yout = np.empty_like(Yin)
    a, b, alpha = f32(a), f32(b), f32(alpha)
    two_ab, two_b, bm1 = f32(f32(2) * a) * b, f32(2) * b, b - f32(1)
    rate = np.asarray(rate, dtype=f32)
    due = np.floor(f32(epoch + 1) * rate) > np.floor(f32(epoch) * rate)
    E = len(indices)
    e = np.arange(E, dtype=np.uint64)
    words = [philox4x32_10(np.stack([e & np.uint64(0xffffffff), e >> np.uint64(32), np.full(E, epoch, np.uint64), np.full(E, g, np.uint64)], 1),
                           (seed & 0xffffffff, seed >> 32)) if E else np.zeros((0, 4), np.uint32) for g in (0, 1)]
    for i in range(N):
        y0, y1 = Yin[i]
        for ei in range(int(indptr[i]), int(indptr[i + 1])):
            if not due[ei]:
                continue
            o0, o1 = Yin[indices[ei]]
            for _ in range(2):
                d0, d1 = y0 - o0, y1 - o1
                d2 = _fma32(d0, d0, d1 * d1)
                g = (-two_ab * _powf(d2, bm1)) / (a * _powf(d2, b) + f32(1)) if d2 > 0 else f32(0)
                y0 = y0 + _clip4(g * d0) * alpha
                y1 = y1 + _clip4(g * d1) * alpha
            for s in range(5):
                kk = int(words[s >> 2][ei, s & 3]) % N
                if kk == i:
                    continue
                d0, d1 = y0 - Yin[kk, 0], y1 - Yin[kk, 1]
                d2 = _fma32(d0, d0, d1 * d1)
                if d2 > 0:
                    g = two_b / ((f32(0.001) + d2) * (a * _powf(d2, b) + f32(1)))
                    y0 = y0 + _clip4(g * d0) * alpha
                    y1 = y1 + _clip4(g * d1) * alpha
                else:
                    y0 = y0 + f32(4) * alpha
                    y1 = y1 + f32(4) * alpha
        Yout[i] = (y0, y1)
    return Yout


def blobs(N, D, n_blobs, seed, spread=12.0):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((n_blobs, D)) * spread
    lab = rng.integers(0, n_blobs, N)
    return (cent[lab] + rng.standard_normal((N, D))).astype(np.float32), lab


def _run_knn(X, k, dev):
    N, D = X.shape
    idx = torch.empty(N, k, dtype=torch.int32, device=dev)
    dist = torch.empty(N, k, device=dev)
    ops.knn(T_(X, dev), N, D, k, idx, dist)
    return N_(idx), N_(dist)


# ------------------------------------------------------------------ kernel cases
def check_knn(dev, N, D, k, seed=0, n_check=None):
    """n_check: compare only that many sampled rows (the large GPU shape)"""
    X = blobs(N, D, 4, seed, spread=3.0)[0]
    idx, dist = _run_knn(X, k, dev)
    rows = np.arange(N) if n_check is None else np.sort(np.random.default_rng(seed).choice(N, n_check, replace=False))
    check_knn_rows(X, idx, dist, rows, k)


def check_knn_duplicates(dev):
    """exact duplicates: the point itself keeps slot 0, its copies follow at distance 0 by ascending index"""
    rng = np.random.default_rng(1)
    X = rng.standard_normal((300, 7)).astype(np.float32)
    copies = [5, 17, 40, 299]
    X[copies] = X[5]
    X[[100, 101]] = X[200]
    idx, dist = _run_knn(X, 6, dev)
    for i in copies:
        others = [c for c in copies if c != i]
        assert idx[i, 0] == i
        assert idx[i, 1:4].tolist() == others, (i, idx[i])
        assert (dist[i, :4] == 0).all() and dist[i, 4] > 0
    assert idx[200, :3].tolist() == [200, 100, 101] and idx[101, :3].tolist() == [101, 100, 200]
    check_knn_rows(X, idx, dist, np.arange(300), 6)


def check_knn_errors(dev):
    from vame_amd import _lib
    L = _lib.lib()
    x = torch.zeros(64, device=dev)
    ii = torch.zeros(64, dtype=torch.int32, device=dev)
    assert L.vame_knn_f32(x.data_ptr(), 8, 65, 2, ii.data_ptr(), x.data_ptr(), None) == -4 and b"D=65" in L.vame_last_error()
    assert L.vame_knn_f32(x.data_ptr(), 300, 2, 257, ii.data_ptr(), x.data_ptr(), None) == -4
    assert L.vame_knn_f32(x.data_ptr(), 300, 2, 1, ii.data_ptr(), x.data_ptr(), None) == -4
    assert L.vame_knn_f32(x.data_ptr(), 4, 2, 5, ii.data_ptr(), x.data_ptr(), None) == -2
    assert L.vame_knn_f32(x.data_ptr(), 1 << 24, 2, 200, ii.data_ptr(), x.data_ptr(), None) == -2 and b"2^31" in L.vame_last_error()
    assert L.vame_knn_f32(None, 8, 2, 2, ii.data_ptr(), x.data_ptr(), None) == -1
    assert L.vame_umap_epoch_f32(x.data_ptr(), x.data_ptr(), 4, ii.data_ptr(), ii.data_ptr(), x.data_ptr(), 0, 1.0, 1.0, 1.0, 0, None) == -1


def _membership(dev, idx, dist):
    N, k = idx.shape
    rho, sigma, w = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, k, device=dev)
    ops.umap_membership(T_(dist, dev), T_(idx, dev), N, k, float(dist.astype(np.float64).mean()), rho, sigma, w)
    return N_(rho), N_(sigma), N_(w)


def check_membership(dev):
    for (N, D, k) in ((300, 30, 15), (260, 5, 200), (200, 3, 2)):
        X = blobs(N, D, 4, 2, spread=3.0)[0]
        X[[7, 8]] = X[9]                                      # two rows whose nearest distances are 0
        idx, dist = _run_knn(X, k, dev)
        rho, sigma, w = _membership(dev, idx, dist)
        r_ref, s_ref, w_ref, conv = membership_ref(dist, idx)
        np.testing.assert_allclose(rho, r_ref, rtol=1e-5)
        np.testing.assert_allclose(sigma, s_ref, rtol=1e-5)
        np.testing.assert_allclose(w, w_ref, rtol=1e-5, atol=1e-7)
        assert (w[np.arange(N), 0] == 0).all()
        assert conv.sum() > N // 2, (k, conv.sum())
        np.testing.assert_allclose(w[conv].astype(np.float64).sum(1), np.log2(k), atol=1e-4)


def _graph(dev, idx, w, n_epochs):
    from vame_amd.analysis.umap_hip import UMAPHIP
    indptr, indices, P = UMAPHIP().graph(T_(idx, dev), T_(w, dev), n_epochs)
    return N_(indptr), N_(indices), N_(P)


def check_graph(dev):
    for (N, D, k, n_epochs) in ((300, 30, 15, 500), (260, 5, 60, 200), (150, 4, 2, 500)):
        X = blobs(N, D, 3, 3, spread=3.0)[0]
        idx, dist = _run_knn(X, k, dev)
        w = _membership(dev, idx, dist)[2]
        indptr, indices, P = _graph(dev, idx, w, n_epochs)
        ref = graph_ref(idx, w, n_epochs)
        np.testing.assert_array_equal(indptr, ref.indptr)
        np.testing.assert_array_equal(indices, ref.indices)
        np.testing.assert_allclose(P, ref.data, rtol=1e-6, atol=1e-7)
        G = sp.csr_matrix((P, indices, indptr), shape=(N, N))
        assert (G != G.T).nnz == 0                            # symmetric, bit for bit


def _epochs(dev, Y0, indptr, indices, P, n_epochs, a, b, seed, first=0):
    Y = T_(np.asarray(Y0, dtype=f32), dev)
    Y2 = torch.empty_like(Y)
    ip, ix, Pt = T_(indptr, dev), T_(indices.astype(np.int32), dev), T_(P.astype(f32), dev)
    rate = Pt / Pt.max()
    for n in range(first, first + n_epochs):
        ops.umap_epoch(Y, Y2, Y.shape[0], ip, ix, rate, n, 1.0 - n / (first + n_epochs), a, b, seed)
        Y, Y2 = Y2, Y
    return N_(Y), N_(rate)


def _epoch_at(dev, Y, csr, n, n_epochs, a, b, seed):
    indptr, indices, P = csr
    Yin = T_(np.asarray(Y, dtype=f32), dev)
    Yout = torch.empty_like(Yin)
    ops.umap_epoch(Yin, Yout, Yin.shape[0], indptr, indices, P / P.max(), n, 1.0 - n / n_epochs, a, b, seed)
    return N_(Yout)


def check_epoch(dev):
    """one epoch (a late one: several edges are not due) from a given layout and seed against the float32 restatement"""
    N, D, k = 300, 30, 15
    X = blobs(N, D, 4, 4, spread=3.0)[0]
    idx, dist = _run_knn(X, k, dev)
    w = _membership(dev, idx, dist)[2]
    indptr, indices, P = _graph(dev, idx, w, 200)
    rng = np.random.default_rng(5)
    Y0 = (rng.random((N, 2)) * 10).astype(f32)
    Y0[11] = Y0[12]                                           # a coincident pair: the d = 0 branches
    seed = 0x1234567887654321
    a, b = 1.577, 0.895
    for epoch in (0, 37):
        Y, rate = _epochs(dev, Y0, indptr, indices, P, 1, a, b, seed, first=epoch)
        ref = epoch_ref(Y0, indptr, indices, rate, epoch, f32(1.0 - epoch / (epoch + 1)), a, b, seed)
        assert_layout_close(Y, ref, f"epoch {epoch}", exact=dev == "cpu")
        assert not np.array_equal(Y, Y0)


def check_pipeline(dev):
    """UMAPHIP.fit at N = 200, D = 8, k = 15, 20 epochs from a given init: every stage against its restatement, chained"""
    from vame_amd.analysis.umap_hip import UMAPHIP, find_ab_params, rescale_0_10
    N, D, k, n_epochs = 200, 8, 15, 20
    X = blobs(N, D, 3, 6, spread=2.0)[0]
    init = np.random.default_rng(7).standard_normal((N, 2)).astype(f32)
    um = UMAPHIP(n_neighbors=k, min_dist=0.1, random_state=42, n_epochs=n_epochs, init=init)
    Y = um.fit_transform(X)
    assert um.init_used_ == "array" and Y.shape == (N, 2) and Y.dtype == f32
    check_knn_rows(X, um.knn_indices_, um.knn_dists_, np.arange(N), k)
    _, _, w, _ = membership_ref(um.knn_dists_, um.knn_indices_)
    G = graph_ref(um.knn_indices_, w, n_epochs)
    Gk = um.graph_
    np.testing.assert_array_equal(Gk.indptr, G.indptr)
    np.testing.assert_array_equal(Gk.indices, G.indices)
    np.testing.assert_allclose(Gk.data, G.data, rtol=1e-5)
    a, b = um.a_, um.b_
    assert (a, b) == find_ab_params(1.0, 0.1) and abs(a - 1.58) < 0.02 and abs(b - 0.90) < 0.02, (a, b)
    # the epochs: each one against the restatement applied to the layout the kernel started it from (the SGD is chaotic where points
    # nearly coincide, so last-ulp differences of powf between libraries are not carried from one epoch into the next), and the chain
    # of launches replayed here gives UMAPHIP's embedding bit for bit
    Yk = rescale_0_10(init)
    rate = (G.data / G.data.max()).astype(f32)
    for n in range(n_epochs):
        Yk_next = _epoch_at(dev, Yk, um._csr, n, n_epochs, a, b, 42)
        ref = epoch_ref(Yk, G.indptr, G.indices, rate, n, f32(1.0 - n / n_epochs), a, b, 42)
        assert_layout_close(Yk_next, ref, f"epoch {n}", exact=dev == "cpu")
        Yk = Yk_next
    np.testing.assert_array_equal(Y, Yk)
    with pytest.raises(ValueError):
        UMAPHIP(n_components=3)


# ------------------------------------------------------------------ vame.visualization
def make_project(root, N, D, n_cluster=5, num_points=30000, n_neighbors=15, amd_gpu_umap=True, seed=0, latents=None):
    """A synthetic project with what visualization() reads: config.yaml, latent_vector_<file>.npy and the motif labels."""
    import yaml
    file = "video-1"
    res = os.path.join(root, "results", file, "VAME", "kmeans-" + str(n_cluster))
    os.makedirs(res, exist_ok=True)
    if latents is None:
        latents, lab = blobs(N, D, n_cluster, seed, spread=4.0)
    else:
        lab = np.random.default_rng(seed).integers(0, n_cluster, latents.shape[0])
    np.save(os.path.join(res, "latent_vector_" + file + ".npy"), latents.astype(f32))
    np.save(os.path.join(res, str(n_cluster) + "_km_label_" + file + ".npy"), lab.astype(np.int64))
    cfg = dict(Project="p", project_path=str(root), model_name="VAME", n_cluster=n_cluster, parameterization="kmeans", all_data="yes",
               video_sets=[file], num_points=num_points, min_dist=0.1, n_neighbors=n_neighbors, random_state=42)
    if amd_gpu_umap is not None:
        cfg["amd_gpu_umap"] = amd_gpu_umap
    cfg_path = os.path.join(root, "config.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    return cfg_path, os.path.join(res, "community", "umap_embedding_" + file + ".npy"), latents


def check_visualization(tmp_path, monkeypatch, N=330, T=30, num_points=250, n_epochs=30):
    """Embedding file of shape (min(num_points, N - T), 2), reuse on the second call, the three label modes, the backend choice and
    the alias.  n_epochs is shortened through UMAPHIP's default here (the emulator runs every epoch on the host)."""
    import vame_amd
    from vame_amd import compat
    from vame_amd.analysis import umap_hip, umap_visualization
    monkeypatch.setattr(umap_hip, "default_epochs", lambda N: n_epochs)
    cfg, out, lat = make_project(tmp_path, N - T, 6, num_points=num_points)
    vame_amd.visualization(cfg)
    emb = np.load(out)
    assert emb.shape == (min(num_points, N - T), 2) and emb.dtype == f32 and np.isfinite(emb).all()
    mtime = os.stat(out).st_mtime_ns

    def no_fit(*a, **kw):
        raise AssertionError("an existing embedding must be reused, not recomputed")
    monkeypatch.setattr(umap_hip.UMAPHIP, "fit", no_fit)
    vame_amd.visualization(cfg, label="motif")
    assert os.stat(out).st_mtime_ns == mtime
    with pytest.raises(FileNotFoundError, match="community"):
        vame_amd.visualization(cfg, label="community")
    comm = os.path.join(os.path.dirname(out), "community_label_video-1.npy")
    np.save(comm, np.arange(N - T) % 3)
    vame_amd.visualization(cfg, label="community")
    umap_visualization._pyplot().close("all")
    # without amd_gpu_umap and without umap-learn: an ImportError that names the key
    cfg2, out2, _ = make_project(tmp_path / "p2", 40, 3, amd_gpu_umap=None)
    try:
        import umap  # noqa: F401
        have_umap = True
    except ImportError:
        have_umap = False
    if not have_umap:
        with pytest.raises(ImportError, match="amd_gpu_umap"):
            vame_amd.visualization(cfg2)
    # the reference's entry point through the alias
    compat.uninstall_alias()
    try:
        top = compat.install_alias()
        assert top.visualization is vame_amd.visualization
        import vame.analysis.umap_visualization as m
        assert m.visualization is vame_amd.visualization
        with pytest.raises(AttributeError):
            top.motif_videos
    finally:
        compat.uninstall_alias()


# ------------------------------------------------------------------ layout quality, determinism, the stock shape (GPU)
def closed_curve(N, D, seed, noise=0.02):
    """A noisy closed curve in D dimensions: three harmonics of equal amplitude, randomly rotated (no 2-D projection unfolds it)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 2 * np.pi, N)
    H = np.stack([np.cos(t), np.sin(t), np.cos(2 * t), np.sin(2 * t), np.cos(3 * t), np.sin(3 * t)], 1)
    Q = np.linalg.qr(rng.standard_normal((D, 6)))[0]
    return (H @ Q.T + noise * rng.standard_normal((N, D))).astype(np.float32), t


def check_layout_blobs(dev):
    """10 well-separated blobs: the kNN graph is disconnected (the random initialisation runs); a 5-NN classifier trained on half of
    the 2-D points predicts the blob of the other half with accuracy >= 0.97"""
    from sklearn.neighbors import KNeighborsClassifier
    from vame_amd.analysis.umap_hip import UMAPHIP
    X, lab = blobs(20000, 30, 10, 11, spread=12.0)
    um = UMAPHIP(n_neighbors=50, min_dist=0.1, random_state=1)
    Y = um.fit_transform(X)
    assert um.init_used_ == "random"
    assert np.isfinite(Y).all()
    acc = KNeighborsClassifier(5).fit(Y[::2], lab[::2]).score(Y[1::2], lab[1::2])
    assert acc >= 0.97, acc
    return acc


def check_layout_curve(dev):
    """a noisy closed curve: the graph is connected (the spectral initialisation runs); trustworthiness (10 neighbours) on 5000 sampled
    points >= 0.90 and above that of a 2-D PCA"""
    from sklearn.decomposition import PCA
    from sklearn.manifold import trustworthiness
    from vame_amd.analysis.umap_hip import UMAPHIP
    X, _ = closed_curve(20000, 30, 12)
    um = UMAPHIP(n_neighbors=50, min_dist=0.1, random_state=2)
    Y = um.fit_transform(X)
    assert um.init_used_ == "spectral"
    s = np.sort(np.random.default_rng(3).choice(len(X), 5000, replace=False))
    tw = trustworthiness(X[s], Y[s], n_neighbors=10)
    tw_pca = trustworthiness(X[s], PCA(2).fit_transform(X)[s], n_neighbors=10)
    assert tw >= 0.90 and tw > tw_pca, (tw, tw_pca)
    return tw, tw_pca


def check_determinism(dev):
    from vame_amd.analysis.umap_hip import UMAPHIP
    X, _ = closed_curve(5000, 30, 13)
    Y1 = UMAPHIP(n_neighbors=30, random_state=42).fit_transform(X)
    um = UMAPHIP(n_neighbors=30, random_state=42)
    Y2 = um.fit_transform(X)
    Y3 = UMAPHIP(n_neighbors=30, random_state=43).fit_transform(X)
    assert um.init_used_ == "spectral"
    np.testing.assert_array_equal(Y1, Y2)
    assert not np.array_equal(Y1, Y3)


def check_visualization_stock(tmp_path):
    """vame.visualization() at the stock num_points 30000, n_neighbors 200, min_dist 0.1 on (40000, 30) latents"""
    import vame_amd
    from vame_amd.analysis.umap_hip import UMAPHIP
    from vame_amd.analysis.umap_visualization import _pyplot
    lat = blobs(40000, 30, 8, 21, spread=3.0)[0]
    cfg, out, lat = make_project(tmp_path, 0, 0, n_cluster=8, num_points=30000, n_neighbors=200, latents=lat)
    vame_amd.visualization(cfg, label="motif")
    _pyplot().close("all")
    emb = np.load(out)
    assert emb.shape == (30000, 2) and emb.dtype == f32 and np.isfinite(emb).all()
    ref = UMAPHIP(n_neighbors=200, min_dist=0.1, random_state=42).fit_transform(lat[:30000])
    np.testing.assert_array_equal(emb, ref)
