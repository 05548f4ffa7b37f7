"""UMAP of the latent vectors on the MI355X (opt-in: cfg['amd_gpu_umap']).

The reference embeds the latents with umap-learn (`umap.UMAP(n_components=2, min_dist, n_neighbors, random_state)`,
vame/analysis/umap_visualization.py:87-94).  This class follows UMAP as published (McInnes, Healy, Melville 2018, arXiv:1802.03426)
with umap-learn's defaults: exact Euclidean kNN (`vame_knn_f32`), smooth-kNN calibration and membership weights
(`vame_umap_membership_f32`), the fuzzy union P = W + W^T - W o W^T (`vame_umap_fuzzy_union_f32`, then torch sort / cumsum build the
CSR), pruning below max(P) / n_epochs, a spectral initialisation on the host (scipy eigsh, a one-off step) and the edge-sampled SGD
layout, one deterministic HIP launch per epoch (`vame_umap_epoch_f32`).  It is NOT bit-identical to umap-learn (exact instead of
approximate neighbours, a different random generator, a gather-form epoch), which is why the default path of `visualization()` stays
on umap-learn when it is installed.  For a given `random_state` the result is bitwise reproducible.
"""
import numpy as np
import torch

from .. import _lib, ops


def find_ab_params(spread, min_dist):
    """a, b of the low-dimensional similarity 1 / (1 + a d^(2b)), least-squares fitted to the offset exponential that min_dist and
    spread define (as umap-learn fits them)."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def default_epochs(N):
    return 500 if N <= 10000 else 200


def rescale_0_10(Y):
    """Every initialisation goes into [0, 10] per dimension before the epochs."""
    Y = np.asarray(Y, dtype=np.float64)
    lo, hi = Y.min(0), Y.max(0)
    span = np.where(hi > lo, hi - lo, 1.0)
    return (10.0 * (Y - lo) / span).astype(np.float32)


class UMAPHIP:
    def __init__(self, n_neighbors=15, n_components=2, min_dist=0.1, random_state=None, n_epochs=None, init="spectral"):
        if n_components != 2:
            raise ValueError(f"UMAPHIP embeds into 2 dimensions only (n_components={n_components})")
        self.n_neighbors, self.n_components, self.min_dist = int(n_neighbors), n_components, float(min_dist)
        self.random_state, self.n_epochs, self.init = random_state, n_epochs, init
        self._graph = None

    # ------------------------------------------------------------------ helpers
    def _dev(self, X):
        t = X if torch.is_tensor(X) else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
        return t.to(device=_lib.device(), dtype=torch.float32).contiguous()

    def _seed(self):
        rs = self.random_state
        if rs is None:
            return int(np.random.SeedSequence().entropy) & 0xffffffffffffffff
        if isinstance(rs, np.random.RandomState):
            return int(rs.randint(0, 2 ** 31 - 1))
        return int(rs) & 0xffffffffffffffff

    # ------------------------------------------------------------------ stages (fit() runs them in order; tools/umap_bench.py times them)
    def knn(self, Xd, k):
        N, D = Xd.shape
        idx = torch.empty(N, k, dtype=torch.int32, device=Xd.device)
        dist = torch.empty(N, k, device=Xd.device)
        ops.knn(Xd, N, D, k, idx, dist)
        return idx, dist

    def membership(self, idx, dist):
        N, k = idx.shape
        rho, sigma, w = torch.empty(N, device=idx.device), torch.empty(N, device=idx.device), torch.empty(N, k, device=idx.device)
        ops.umap_membership(dist, idx, N, k, float(dist.double().mean()), rho, sigma, w)
        return rho, sigma, w

    def graph(self, idx, w, n_epochs):
        """Symmetric CSR (both directions of every edge), entries below max(P) / n_epochs dropped: (indptr int64, indices int32, P)."""
        N, k = idx.shape
        dev = idx.device
        p = torch.empty(N, k, device=dev)
        rev = torch.empty(N, k, dtype=torch.int32, device=dev)
        ops.umap_fuzzy_union(idx, w, N, k, p, rev)
        rows = torch.arange(N, device=dev).repeat_interleave(k)
        cols, pv, rv = idx.reshape(-1).long(), p.reshape(-1), rev.reshape(-1)
        keep = (cols != rows) & (pv > 0)
        back = keep & (rv == 0)                       # (j, i) of a pair that only row i holds
        r = torch.cat([rows[keep], cols[back]])
        c = torch.cat([cols[keep], rows[back]])
        v = torch.cat([pv[keep], pv[back]])
        vmax = v.max()
        m = v >= vmax / n_epochs
        r, c, v = r[m], c[m], v[m]
        order = torch.argsort(r * N + c)              # unique keys: one order
        r, c, v = r[order], c[order], v[order]
        indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        indptr[1:] = torch.cumsum(torch.bincount(r, minlength=N), 0)
        return indptr, c.to(torch.int32), v

    def initial(self, N, seed):
        """(N, 2) float32 in [0, 10]; sets init_used_ to 'spectral', 'random' or 'array'."""
        init = self.init
        gen = np.random.Generator(np.random.Philox(seed))
        if isinstance(init, str) and init == "spectral":
            from scipy.sparse.csgraph import connected_components
            G = self.graph_
            n_comp, _ = connected_components(G, directed=False)
            emb = None
            if n_comp > 1:
                print(f"UMAPHIP: the kNN graph has {n_comp} connected components; using a uniform random initialisation instead of the "
                      "spectral one")
            elif N < 5:
                print("UMAPHIP: too few points for a spectral initialisation; using a uniform random one")
            else:
                emb = self._spectral(G)
                if emb is None:
                    print("UMAPHIP: the eigensolver did not converge; using a uniform random initialisation")
            if emb is not None:
                self.init_used_ = "spectral"
                emb = emb * (10.0 / np.abs(emb).max()) + gen.normal(scale=1e-4, size=emb.shape)
                return rescale_0_10(emb)
            init = "random"
        if isinstance(init, str) and init == "random":
            self.init_used_ = "random"
            return rescale_0_10(gen.uniform(-10.0, 10.0, size=(N, 2)))
        if isinstance(init, str):
            raise ValueError(f"init must be 'spectral', 'random' or an (N, 2) array, not {init!r}")
        Y = np.asarray(init, dtype=np.float32)
        if Y.shape != (N, 2):
            raise ValueError(f"init array has shape {Y.shape}, expected ({N}, 2)")
        self.init_used_ = "array"
        return rescale_0_10(Y)

    @staticmethod
    def _spectral(G):
        """Eigenvectors of the 2nd and 3rd smallest eigenvalues of I - D^-1/2 P D^-1/2, i.e. the 2nd and 3rd largest of D^-1/2 P D^-1/2."""
        import scipy.sparse as sp
        from scipy.sparse.linalg import ArpackNoConvergence, eigsh
        N = G.shape[0]
        deg = np.asarray(G.sum(axis=1), dtype=np.float64).ravel()
        Dm = sp.diags(1.0 / np.sqrt(deg))
        A = (Dm @ G.astype(np.float64) @ Dm).tocsr()
        try:
            vals, vecs = eigsh(A, k=3, which="LA", ncv=min(N, max(2 * 3 + 1, int(np.sqrt(N)))), tol=1e-4, v0=np.ones(N), maxiter=N * 5)
        except ArpackNoConvergence:
            return None
        order = np.argsort(vals)[::-1]
        return vecs[:, order[1:3]]

    def layout(self, Y0, indptr, indices, P, n_epochs, seed):
        N = Y0.shape[0]
        a, b = find_ab_params(1.0, self.min_dist)
        self.a_, self.b_ = a, b
        rate = P / P.max()
        Y = torch.from_numpy(np.ascontiguousarray(Y0, dtype=np.float32)).to(indptr.device)
        Y2 = torch.empty_like(Y)
        for n in range(n_epochs):
            ops.umap_epoch(Y, Y2, N, indptr, indices, rate, n, 1.0 - n / n_epochs, a, b, seed)
            Y, Y2 = Y2, Y
        return Y

    # ------------------------------------------------------------------ umap-learn-like API
    @property
    def graph_(self):
        """The pruned fuzzy graph as a scipy CSR matrix on the host (built on first use)."""
        if self._graph is None:
            import scipy.sparse as sp
            indptr, indices, P = self._csr
            N = indptr.numel() - 1
            self._graph = sp.csr_matrix((P.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=(N, N))
        return self._graph

    def fit(self, X):
        Xd = self._dev(X)
        N = Xd.shape[0]
        if N < 2:
            raise ValueError(f"UMAPHIP needs at least 2 points (got {N})")
        k = min(self.n_neighbors, N)
        n_epochs = int(self.n_epochs) if self.n_epochs is not None else default_epochs(N)
        seed = self._seed()
        self._graph = None
        idx, dist = self.knn(Xd, k)
        _, _, w = self.membership(idx, dist)
        self._csr = self.graph(idx, w, n_epochs)
        Y0 = self.initial(N, seed)
        Y = self.layout(Y0, *self._csr, n_epochs, seed)
        self.knn_indices_, self.knn_dists_ = idx.cpu().numpy(), dist.cpu().numpy()
        self.embedding_ = Y.cpu().numpy()
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_
