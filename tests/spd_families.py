"""Seeded families of symmetric positive definite test matrices, and the factor comparison the GPU tests use.  Host only.

Every dense fp32 test of the factorisation used to build its matrix as K[i,j] = V[min(i,j)] + sigma^2 I (the volatility kernel,
voltron/kernels/VolKernel.py:30-33).  Below the diagonal a column of that matrix is constant, and by induction so is every
column of its Cholesky factor: an off-diagonal 128-block of L, of L^-1 and of K_s^-1 has rank ONE, and a kernel that reads or
writes the wrong ROW of such a block (a wrong row block of a panel, an LDS row swizzle, a mixed-up accumulator row) still
produces the right factor.  The families here have no such structure:

  wishart        G G'/N + I, G ~ N(0,1): condition number ~5, every off-diagonal block of L of full rank;
  rbf_irregular  exp(-(t_i - t_j)^2 / (2 0.3^2)) + 0.05 I, t sorted uniform on [0,4]: condition number 1e3 .. 2.4e3, the regime
                 the project's fp32 tolerances are stated for;
  scaled         D (G G'/N + I) D, D = diag(10^U(-1.5,1.5)): pivots over three decades (condition number ~1e6);
  vol            the volatility kernel + sigma^2 I itself, the control.

Each generator returns fp64 [B,N,N] whose entries are exactly representable in `dtype` (generated in fp64, rounded through
it): the kernel under test and the fp64 reference see the same numbers.  The matrices are exactly symmetric."""
import numpy as np

FAMILIES = ("wishart", "rbf_irregular", "scaled", "vol")
GENERIC = ("wishart", "rbf_irregular", "scaled")
TILE = 128                                            # the kernels' block size (volt_amd.ops.TILE)
RBF_LENGTHSCALE, RBF_NOISE, RBF_SPAN = 0.3, 0.05, 4.0
SCALED_DECADES = 1.5


def _np_dtype(dtype):
    s = str(dtype)                                    # numpy or torch dtypes, or their names
    if "float32" in s:
        return np.float32
    if "float64" in s:
        return np.float64
    raise ValueError(f"fp32 or fp64 (got {dtype})")


def _rng(tag, B, N, seed):
    return np.random.default_rng([FAMILIES.index(tag), B, N, seed])


def _through(A, dtype):
    A = 0.5 * (A + np.swapaxes(A, -1, -2))            # exactly symmetric before and therefore after the rounding
    return A.astype(_np_dtype(dtype)).astype(np.float64)


def _gram(rng, B, N):
    G = rng.standard_normal((B, N, N))
    return G @ np.swapaxes(G, -1, -2) / N + np.eye(N)


def wishart(B, N, dtype=np.float32, seed=0):
    return _through(_gram(_rng("wishart", B, N, seed), B, N), dtype)


def rbf_irregular(B, N, dtype=np.float32, seed=0):
    t = np.sort(_rng("rbf_irregular", B, N, seed).uniform(0.0, RBF_SPAN, size=(B, N)), axis=-1)
    d = t[:, :, None] - t[:, None, :]
    return _through(np.exp(-0.5 * (d / RBF_LENGTHSCALE) ** 2) + RBF_NOISE * np.eye(N), dtype)


def scaled(B, N, dtype=np.float32, seed=0):
    rng = _rng("scaled", B, N, seed)
    D = 10.0 ** rng.uniform(-SCALED_DECADES, SCALED_DECADES, size=(B, N))
    return _through(D[:, :, None] * _gram(rng, B, N) * D[:, None, :], dtype)


def vol(B, N, dtype=np.float32, seed=0):
    """K = fill(cumtrapz(vol^2)) + sigma^2 I on the suite's own series (volt_amd.synthetic.sde_batch) and noise."""
    from oracle import volt_oracle as vo
    from volt_amd.synthetic import sde_batch
    x, _F, v = sde_batch(B, N, 2019 + seed)
    x, v = x.astype(np.float64), v.astype(np.float64)
    K = vo.volatility_kernel(np.repeat(x[None], B, 0)[..., None], v[..., None])
    return _through(K + float(vo.noise_from_raw(1e-5)) * np.eye(N), dtype)


def make(family, B, N, dtype=np.float32, seed=0):
    if family not in FAMILIES:
        raise ValueError(f"unknown family {family!r}")
    return globals()[family](B, N, dtype, seed)


def rhs(B, N, dtype=np.float32, seed=0):
    """A right-hand side [B,N] ~ N(0,1), fp64 rounded through `dtype`."""
    r = np.random.default_rng([len(FAMILIES), B, N, seed]).standard_normal((B, N))
    return r.astype(_np_dtype(dtype)).astype(np.float64)


# ------------------------------------------------------------------ the comparison
def factor_error(L, L_ref, A):
    """max_ij |L_ij - Lref_ij| / sqrt(A_ii) over the whole batch: row i of a Cholesky factor has 2-norm sqrt(A_ii), so this is
    the error of every entry relative to its own ROW -- a small row of `scaled` is not hidden behind the large ones."""
    L, L_ref, A = (np.asarray(t, dtype=np.float64) for t in (L, L_ref, A))
    if L.shape != L_ref.shape or L.shape != A.shape:
        raise ValueError(f"shapes disagree: {L.shape} {L_ref.shape} {A.shape}")
    d = np.abs(np.tril(L) - np.tril(L_ref))
    if not np.isfinite(d).all():
        return float("inf")
    row = np.sqrt(np.diagonal(A, axis1=-2, axis2=-1))
    return float((d / row[..., :, None]).max())


def assert_factor_close(L, L_ref, A, tol=2e-5, what=""):
    """The lower triangles of L and L_ref agree to `tol` on the row-normalised measure of `factor_error`.  Returns the error."""
    err = factor_error(L, L_ref, A)
    assert err <= tol, f"{what} factor error {err:.3e} of its row's norm > {tol:.1e}"
    return err


def block_rank(M, rtol=1e-10):
    """Numerical rank of a block: singular values above rtol of the largest."""
    s = np.linalg.svd(np.asarray(M, dtype=np.float64), compute_uv=False)
    return int((s > rtol * s[0]).sum())


def permute_block_rows(L, rows, cols, perm):
    """A copy of L [B,N,N] with the rows of the block L[:, rows, cols] (two slices) taken in the order `perm`: what a tile that
    reads or writes the wrong row of an off-diagonal block produces."""
    out = np.array(L, dtype=np.float64, copy=True)
    blk = out[:, rows, cols].copy()
    out[:, rows, cols] = blk[:, np.asarray(perm), :]
    return out


# ------------------------------------------------------------------ fp64 references (host LAPACK)
def reference(A, r=None, keep_y=False):
    """fp64 LAPACK quantities of A [B,N,N] (and r [B,N]): L; with r also z = L^-1 r, alpha = A^-1 r and the columns of the
    MLL step's `out` (include/volt_hip.h): mll, dsig = d mll / d sigma2, quad = r'A^-1 r, logdet, trinv = tr A^-1,
    aa = alpha'alpha; keep_y: also Y = L^-T [B,N,N]."""
    from scipy.linalg import solve_triangular
    A = np.asarray(A, dtype=np.float64)
    B, N, _ = A.shape
    L = np.linalg.cholesky(A)
    ref = dict(L=L)
    if r is None:
        return ref
    eye = np.eye(N)
    alpha, z, trinv = np.empty((B, N)), np.empty((B, N)), np.empty(B)
    Ys = np.empty((B, N, N)) if keep_y else None
    for b in range(B):
        z[b] = solve_triangular(L[b], r[b], lower=True)
        alpha[b] = solve_triangular(L[b], z[b], lower=True, trans="T")
        Y = solve_triangular(L[b], eye, lower=True).T              # L^-T, upper
        trinv[b] = (Y * Y).sum()
        if keep_y:
            Ys[b] = Y
    quad = (z * z).sum(-1)
    logdet = 2.0 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum(-1)
    aa = (alpha * alpha).sum(-1)
    if keep_y:
        ref["Y"] = Ys
    ref.update(alpha=alpha, z=z, quad=quad, logdet=logdet, trinv=trinv, aa=aa,
               mll=-0.5 * (quad + logdet + N * np.log(2.0 * np.pi)) / N, dsig=0.5 * (aa - trinv) / N)
    return ref
