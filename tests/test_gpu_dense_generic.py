"""The dense Cholesky paths on matrices whose factor is NOT rank-one below the diagonal (tests/spd_families.py) -- needs an MI355X.

Every other dense test factors the volatility kernel K[i,j] = V[min(i,j)] + sigma^2 I (or the Brownian-motion prior, which has
the same structure): below the diagonal a column of its factor is constant, so a tile that reads or writes the wrong ROW of an
off-diagonal block -- a wrong row block of a panel, an LDS row swizzle, a mixed-up accumulator row -- still gives the right
factor, alpha and MLL, and the bitwise one-launch / launch-per-column comparisons share the tile bodies (tests/test_spd_families_host.py
shows both halves of that on the host).  Here every schedule of the step factors `wishart` (full-rank blocks, cond ~5),
`rbf_irregular` (cond ~3.8 N: 1e3 at N = 257, 1e4 at N = 2561) and, at one shape per schedule, `scaled` (rows over three
decades, cond ~1e6), against fp64 LAPACK (numpy on the host up to N = 1300, torch in double on the device above), ALL batch
entries.

What is compared per step: the factor the step left in its workspace (csrc/mll.hip carve(): A is the workspace's first
region) on the row-normalised measure max |L - L64|_ij / sqrt(A_ii); out[:, 0..5]; alpha.  Tolerances are the project's
existing ones for cond <= 3e3, unchanged: factor 2e-5, MLL 2e-5, tr K_s^-1 and alpha'alpha 1e-4 (quad: the 1e-4 of
test_gpu_lownoise.py; logdet: 2e-5 of max(N, |logdet|), what the MLL's tolerance leaves it), alpha / trsv / trtri 1e-4 of the
maximum, d/d sigma^2 1e-3 with the floor of test_randomised_sizes_batches_and_noise_against_oracle; fp64 1e-10 up to N = 1024
and 1e-9 above, 100 x that for alpha and the gradient.  `scaled`: factor and alpha only, <= 3 x the error of the vendor's fp32
torch.linalg.cholesky + triangular solves on the same matrix (floors 3e-7 / 2e-6, as test_gpu_lownoise.py).  The dense gradient
volt_mll_grad_k_f32 is held to 1e-3 of its largest entry: its trace is N d mll / d sigma^2, gated at 1e-3.

Which schedule ran is asserted where the library has a hook: volt_profile_step_f32's launch counts ([1, 0] is the batched
one-launch step, anything else a launch per block column), volt_potrf_workspace_bytes(_f64) > 0, tables=False.  The short- and
long-series one-launch steps have no hook; their shapes are those of small_applies / long_applies (csrc/one_launch.hip) and the
profile hook confirms that the batched step does not take them.

Only the lower triangle of K is read (include/volt_hip.h: volt_potrf_k_f32, volt_potrf_k_f64; the MLL step unless
VOLT_REFINE_ALPHA): the strict upper triangle filled with NaN must give info = 0 and the same bits.

Every case prints its figures before it asserts (GENERIC ...).  Worst measured, MI355X (family: factor / mll / alpha):
    path                      wishart                       rbf_irregular                 scaled (x vendor)
    one block                 3.4e-7 / 4.9e-8 / 6.6e-7      1.9e-6 / 1.7e-6 / 8.8e-6      4.0e-7 / - / 6.0e-7
    short series, one launch  6.6e-7 / 3.6e-8 / 7.5e-7      5.2e-6 / 4.0e-6 / 5.1e-5      5.5e-7 / - / 7.2e-7
    launch per column         5.2e-7 / 3.8e-8 / 5.6e-7      3.6e-6 / 1.8e-6 / 3.0e-5      5.6e-7 / - / 4.9e-7
    table schedules           4.3e-7 / 3.7e-8 / 5.0e-7      4.2e-6 / 8.5e-7 / 3.0e-5      4.7e-7 / - / 5.8e-7
    one long series           5.8e-7 / 2.2e-8 / 5.2e-7      3.9e-6 / 1.5e-6 / 4.3e-5      5.8e-7 / - / 4.9e-7
    batched one launch        5.1e-7 / 3.4e-8 / 6.1e-7      6.1e-6 / 2.8e-6 / 5.0e-5      5.7e-7 / - / 1.0e-6
    ops.potrf (all paths)     6.2e-7                        5.8e-6                        5.8e-7
    fp64 one launch           2.0e-15 / 1.1e-16 / 2.8e-15   2.1e-14 / 1.3e-14 / 2.0e-13
    fp64 launch per column    6.4e-16                       6.5e-15
d/d sigma^2 <= 1.2e-6 (wishart) / 8.0e-6 (rbf_irregular); tr K_s^-1, alpha'alpha <= 7.6e-6; trsv / trtri / cholesky_solve <= 4.7e-7
/ 2.5e-5, grad_K 6.9e-7 / 5.3e-5; `scaled` against the vendor: factor <= 1.36 x, alpha <= 1.38 x its error."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import spd_families as F

pytestmark = pytest.mark.gpu
HOST_REF_NMAX = 1300


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from volt_amd import ops as _ops
    return _ops


def _device_reference(A, r):
    """F.reference in double on the device (N above HOST_REF_NMAX), one matrix at a time."""
    B, N, _ = A.shape
    st = torch.linalg.solve_triangular
    eye = torch.eye(N, device="cuda", dtype=torch.float64)
    keys = ("L", "alpha", "z", "quad", "logdet", "trinv", "aa")
    acc = {k: [] for k in keys}
    for b in range(B):
        Ab, rb = torch.as_tensor(A[b]).cuda(), torch.as_tensor(r[b]).cuda()[:, None]
        L = torch.linalg.cholesky(Ab)
        z = st(L, rb, upper=False)
        al = st(L.mT, z, upper=True)
        Y = st(L, eye, upper=False)
        vals = (L, al[:, 0], z[:, 0], (z * z).sum(), 2 * torch.log(torch.diagonal(L)).sum(), (Y * Y).sum(), (al * al).sum())
        for k, v in zip(keys, vals):
            acc[k].append(v.cpu().numpy())
    ref = {k: np.stack(v) for k, v in acc.items()}
    ref["mll"] = -0.5 * (ref["quad"] + ref["logdet"] + N * np.log(2.0 * np.pi)) / N
    ref["dsig"] = 0.5 * (ref["aa"] - ref["trinv"]) / N
    return ref


@functools.lru_cache(maxsize=2)
def _problem(family, B, N, dtype=torch.float32, keep_y=False):
    """One matrix set per (family, shape), shared by the cases that follow each other on it; never modified."""
    A = F.make(family, B, N, dtype)
    r = F.rhs(B, N, dtype)
    ref = F.reference(A, r, keep_y) if N <= HOST_REF_NMAX else _device_reference(A, r)
    K = torch.as_tensor(A).to(dtype).cuda()
    assert torch.equal(K.double().cpu(), torch.as_tensor(A))           # the kernel sees the reference's numbers
    return dict(A=A, K=K, r=torch.as_tensor(r).to(dtype).cuda(), s2=torch.zeros(B, dtype=dtype, device="cuda"), ref=ref)


def _ws_factor(ws):
    """The factor a step left in its workspace: A [B,Np,Np] is the first region (csrc/mll.hip carve(), csrc/mll64.hip carve64())."""
    from volt_amd import ops
    Np = ops.padded_n(ws.N)
    esz = 4 if ws.dtype == torch.float32 else 8
    off = ws.ptr - ws.buf.data_ptr()
    A = ws.buf[off: off + ws.B * Np * Np * esz].view(ws.dtype).view(ws.B, Np, Np)
    return torch.tril(A[:, : ws.N, : ws.N])


def _launch_counts(ops, p, B, N):
    """volt_profile_step_f32 on an initialised workspace of this shape: launches per kernel class of the step it runs."""
    from volt_amd import _lib
    ws = ops.MllWorkspace(B, N, True, p["K"].device)
    ms_sum, ms_un, cnt = (ctypes.c_float * 2)(), (ctypes.c_float * 2)(), (ctypes.c_int * 2)()
    inf = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().volt_profile_step_f32(p["K"].data_ptr(), N, N * N, p["r"].data_ptr(), p["s2"].data_ptr(), ws.out.data_ptr(),
                                                ws.alpha.data_ptr(), ws.ptr, inf.data_ptr(), B, N, 0, _lib.stream_ptr(), ms_sum,
                                                ms_un, cnt, None), "profile")
    assert int(inf.abs().sum()) == 0
    return list(cnt)


def _vendor_errors(p, b):
    """The yardstick of `scaled`: the vendor's fp32 factorisation + substitution on matrix b, on the same measures."""
    st = torch.linalg.solve_triangular
    Lv = torch.linalg.cholesky(p["K"][b])
    av = st(Lv.mT, st(Lv, p["r"][b][:, None], upper=False), upper=True)[:, 0]
    ref = p["ref"]
    e_l = F.factor_error(Lv.cpu().numpy()[None], ref["L"][b][None], p["A"][b][None])
    e_a = float(np.abs(av.double().cpu().numpy() - ref["alpha"][b]).max() / np.abs(ref["alpha"][b]).max())
    return e_l, e_a


def _alpha_error(alpha, ref):
    a = alpha.double().cpu().numpy()
    return np.abs(a - ref["alpha"]).max(-1) / np.abs(ref["alpha"]).max(-1)          # [B]


def _check(label, family, p, L=None, out=None, alpha=None, forward_only=False, f64=False):
    """Print, then gate, everything a path exposes against the fp64 reference (all batch entries)."""
    ref, A = p["ref"], p["A"]
    B, N = A.shape[0], A.shape[1]
    fig = {}
    if L is not None:
        Lh = L.double().cpu().numpy()
        fig["factor"] = F.factor_error(Lh, ref["L"], A)
    if out is not None:
        o = out.double().cpu().numpy()
        fig["mll"] = float(np.abs(o[:, 0] / ref["mll"] - 1).max())
        fig["quad"] = float(np.abs(o[:, 2] / ref["quad"] - 1).max())
        fig["logdet"] = float((np.abs(o[:, 3] - ref["logdet"]) / np.maximum(N, np.abs(ref["logdet"]))).max())
        if not forward_only:
            fig["dsig"] = float((np.abs(o[:, 1] - ref["dsig"]) / np.maximum(np.abs(ref["dsig"]), 1e-4 * ref["trinv"] / N)).max())
            fig["trinv"] = float(np.abs(o[:, 4] / ref["trinv"] - 1).max())
            fig["aa"] = float(np.abs(o[:, 5] / ref["aa"] - 1).max())
    if alpha is not None:
        fig["alpha"] = float(_alpha_error(alpha, ref).max())
    print("GENERIC", label, family, f"B={B} N={N}", " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    if family == "scaled":                                             # cond ~1e6: held against the vendor's fp32, matrix by matrix
        for b in range(B):
            v_l, v_a = _vendor_errors(p, b)
            e_l = F.factor_error(Lh[b][None], ref["L"][b][None], A[b][None]) if L is not None else 0.0
            e_a = float(_alpha_error(alpha, ref)[b]) if alpha is not None else 0.0
            print("GENERIC", label, family, f"b={b} factor {e_l:.2e} (vendor {v_l:.2e})" + (f" alpha {e_a:.2e} (vendor {v_a:.2e})" if alpha is not None else ""))
            assert e_l <= 3 * max(v_l, 3e-7), (label, b, "factor vs vendor", e_l, v_l)
            assert e_a <= 3 * max(v_a, 2e-6), (label, b, "alpha vs vendor", e_a, v_a)
        return fig
    t = (1e-10 if N <= 1024 else 1e-9) if f64 else None
    tol = dict(factor=t, mll=t, quad=t, logdet=t, dsig=100 * t, trinv=100 * t, aa=100 * t, alpha=100 * t) if f64 else \
        dict(factor=2e-5, mll=2e-5, quad=1e-4, logdet=2e-5, dsig=1e-3, trinv=1e-4, aa=1e-4, alpha=1e-4)
    bad = {k: (v, tol[k]) for k, v in fig.items() if not v <= tol[k]}
    assert not bad, (label, family, B, N, bad)
    return fig


# ------------------------------------------------------------------ the fp32 gradient step, schedule by schedule
# (path, B, N): the smallest shapes that reach each schedule (csrc/one_launch.hip small_applies / long_applies,
# csrc/batch_step.hip volt_internal_batch_applies); cases on one shape follow each other and share its reference
STEP_SHAPES = [("diag", 2, 100), ("diag", 2, 128),                     # one diagonal block
               ("short", 3, 257), ("percol", 3, 257),                  # three block columns, one row in the last
               ("short", 5, 512), ("percol", 5, 512),
               ("short", 2, 1024), ("percol", 2, 1024),
               ("percol", 9, 640),
               ("table", 4, 1100),                                     # 9 block columns: neither short nor batched
               ("long", 1, 385), ("long", 1, 1153),
               ("batch", 20, 1024), ("batch", 6, 1280), ("batch", 8, 1280), ("batch", 2, 2561)]
SCALED_AT = {("diag", 2, 128), ("short", 3, 257), ("percol", 9, 640), ("table", 4, 1100), ("long", 1, 1153), ("batch", 6, 1280)}
STEP_CASES = [(path, B, N, fam) for (path, B, N) in STEP_SHAPES for fam in F.GENERIC
              if fam != "scaled" or (path, B, N) in SCALED_AT]


@pytest.mark.parametrize("path,B,N,family", STEP_CASES)
def test_gradient_step_matches_fp64_on_generic_matrices(ops, path, B, N, family):
    p = _problem(family, B, N)
    ws = ops.MllWorkspace(B, N, True, p["K"].device)
    out, alpha, info = ops.mll_step(p["K"], p["r"], p["s2"], ws, tables=(path != "percol"))
    assert int(info.abs().sum()) == 0, info
    _check(path, family, p, L=_ws_factor(ws), out=out, alpha=alpha)
    if path != "percol":
        cnt = _launch_counts(ops, p, B, N)
        assert (cnt == [1, 0]) == (path == "batch"), (path, B, N, cnt)
        if path == "table":
            assert cnt[0] >= ops.padded_n(N) // 128, cnt               # a launch per block column


def test_batched_one_launch_step_is_bitwise_the_launch_per_column_step_on_full_rank_data(ops):
    """8 matrices: the uninitialised workspace runs the plain table-free schedule, which sums the way the one launch does
    (tests/test_gpu_batch_step.py) -- on the volatility kernel that comparison cannot see a wrong row, here it can."""
    from test_gpu_batch_step import _plain_reference
    B, N = 8, 1280
    p = _problem("wishart", B, N)
    ws = ops.MllWorkspace(B, N, True, p["K"].device)
    out, alpha, info = ops.mll_step(p["K"], p["r"], p["s2"], ws)
    assert int(info.abs().sum()) == 0
    out, alpha = out.clone(), alpha.clone()
    out2, alpha2 = _plain_reference(ops, p["K"], p["r"], p["s2"], B, N)
    assert torch.equal(out, out2) and torch.equal(alpha, alpha2)


@pytest.mark.parametrize("B,N,family", [(3, 640, "wishart"), (3, 640, "rbf_irregular"), (1, 1153, "wishart"), (1, 1153, "rbf_irregular")])
def test_forward_only_step_on_generic_matrices(ops, B, N, family):
    """want_grad = False (potrf + the one-launch TRSV): mll and quad against fp64 and against the gradient path."""
    p = _problem(family, B, N)
    ws = ops.MllWorkspace(B, N, False, p["K"].device)
    o0, _a, info = ops.mll_step(p["K"], p["r"], p["s2"], ws, want_grad=False)
    assert int(info.abs().sum()) == 0
    _check("forward", family, p, L=_ws_factor(ws), out=o0, forward_only=True)
    o1, _a, info = ops.mll_step(p["K"], p["r"], p["s2"], want_grad=True)
    assert int(info.abs().sum()) == 0
    assert torch.allclose(o1[:, 0], o0[:, 0], rtol=1e-5) and torch.allclose(o1[:, 2], o0[:, 2], rtol=1e-4)


# ------------------------------------------------------------------ the factorisation alone
POTRF_SHAPES = [("diag", 2, 100, True), ("small", 3, 257, True), ("percol", 3, 257, False), ("small", 2, 1024, True),
                ("percol", 9, 640, False), ("table", 4, 1100, True), ("batch", 8, 1280, True), ("batch", 24, 1024, True)]
POTRF_SCALED_AT = {("small", 3, 257), ("percol", 9, 640), ("batch", 8, 1280)}


@pytest.mark.parametrize("path,B,N,tables,family", [(pa, B, N, t, fam) for (pa, B, N, t) in POTRF_SHAPES for fam in F.GENERIC
                                                    if fam != "scaled" or (pa, B, N) in POTRF_SCALED_AT])
def test_potrf_matches_fp64_on_generic_matrices(ops, path, B, N, tables, family):
    """ops.potrf -> volt_potrf_k_f32: (8, 1280) and (24, 1024) are the has_y = 0 gates of the batched one launch."""
    p = _problem(family, B, N)
    if path == "batch":
        assert ops._potrf_workspace(B, ops.padded_n(N), p["K"].device)[0] is not None
    f = ops.potrf(p["K"], tables=tables)
    assert int(f.info.abs().sum()) == 0
    _check("potrf-" + path, family, p, L=f.L)
    if path == "batch":                                                # bitwise the plain launch-per-column schedule (8 / 24 matrices)
        f2 = ops.potrf(p["K"], tables=False)
        assert torch.equal(f2.L, f.L) and torch.equal(f2.Winv, f.Winv)


# ------------------------------------------------------------------ stand-alone primitives on a generic factor
@pytest.mark.parametrize("N", [300, 640])
@pytest.mark.parametrize("family", ["wishart", "rbf_irregular"])
def test_primitives_on_a_generic_factor(ops, family, N):
    from scipy.linalg import solve_triangular
    B = 2
    p = _problem(family, B, N, torch.float32, True)
    ref, A = p["ref"], p["A"]
    f = ops.potrf(p["K"])
    assert int(f.info.abs().sum()) == 0
    rel = lambda got, want: float(np.abs(got.double().cpu().numpy() - want).max() / np.abs(want).max())
    zt = np.stack([solve_triangular(ref["L"][b], p["r"][b].double().cpu().numpy(), lower=True, trans="T") for b in range(B)])
    fig = dict(trsv=rel(ops.trsv(f, p["r"], check=True), ref["z"]), trsv_t=rel(ops.trsv(f, p["r"], transpose=True, check=True), zt),
               solve=rel(ops.cholesky_solve(f, p["r"]), ref["alpha"]), trtri=rel(ops.trtri(f), ref["Y"]))
    ws = ops.MllWorkspace(B, N, True, p["K"].device)
    _o, alpha, info = ops.mll_step(p["K"], p["r"], p["s2"], ws)
    assert int(info.abs().sum()) == 0
    gK_ref = 0.5 * (ref["alpha"][:, :, None] * ref["alpha"][:, None, :] - ref["Y"] @ np.swapaxes(ref["Y"], -1, -2)) / N
    fig["grad_k"] = rel(ops.mll_grad_k(ws), gK_ref)
    print("GENERIC primitives", family, f"B={B} N={N}", " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert max(fig["trsv"], fig["trsv_t"], fig["solve"], fig["trtri"]) <= 1e-4, fig
    assert fig["grad_k"] <= 1e-3, fig


# ------------------------------------------------------------------ fp64
@pytest.mark.parametrize("B,N", [(4, 256), (5, 300), (3, 1000)])
@pytest.mark.parametrize("family", ["wishart", "rbf_irregular"])
def test_fp64_one_launch_on_generic_matrices(ops, family, B, N):
    from volt_amd import _lib
    assert _lib.lib().volt_potrf_workspace_bytes_f64(B, ops.padded_n(N)) > 0, "the shape must run as one launch"
    p = _problem(family, B, N, torch.float64)
    f = ops.potrf(p["K"])
    assert int(f.info.abs().sum()) == 0
    _check("potrf64", family, p, L=f.L, f64=True)
    ws = ops.MllWorkspace(B, N, True, p["K"].device, torch.float64)
    out, alpha, info = ops.mll_step(p["K"], p["r"], p["s2"], ws)
    assert int(info.abs().sum()) == 0
    _check("step64", family, p, L=_ws_factor(ws), out=out, alpha=alpha, f64=True)


@pytest.mark.parametrize("family", ["wishart", "rbf_irregular"])
def test_fp64_launch_per_column_and_trsv_on_generic_matrices(ops, family):
    """A null workspace is volt_potrf_f64, the launch-per-column path (tests/test_gpu_batch64.py); the fp64 solves at N = 300."""
    from volt_amd import _lib
    L = _lib.lib()
    B, N = 3, 640
    p = _problem(family, B, N, torch.float64)
    K = p["K"]
    Np = ops.padded_n(N)
    A = torch.empty(B, Np, Np, dtype=torch.float64, device="cuda")
    W = torch.empty(B, Np // 128, 128, 128, dtype=torch.float64, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(L.volt_prepare_f64(K.data_ptr(), N, N * N, None, 0.0, A.data_ptr(), B, N, _lib.stream_ptr()), "prep")
    _lib.check(L.volt_potrf_ws_f64(A.data_ptr(), W.data_ptr(), info.data_ptr(), B, Np, None, 0, _lib.stream_ptr()), "potrf")
    assert int(info.abs().sum()) == 0
    _check("potrf64-percol", family, p, L=torch.tril(A[:, :N, :N]), f64=True)
    B, N = 2, 300
    p = _problem(family, B, N, torch.float64)
    f = ops.potrf(p["K"])
    assert int(f.info.abs().sum()) == 0
    rel = lambda got, want: float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max())
    e_z, e_a = rel(ops.trsv(f, p["r"], check=True), p["ref"]["z"]), rel(ops.cholesky_solve(f, p["r"]), p["ref"]["alpha"])
    print("GENERIC trsv64", family, f"B={B} N={N} trsv={e_z:.2e} solve={e_a:.2e}")
    assert e_z <= 1e-8 and e_a <= 1e-8                                 # (100 x the factor's 1e-10, as alpha's)


# ------------------------------------------------------------------ only the lower triangle of K is read
def _poisoned(K, pad=0):
    """K with NaN in its strict upper triangle; pad > 0: as a strided view (row stride N + pad) of a buffer whose padding is NaN too."""
    B, N, _ = K.shape
    buf = torch.full((B, N, N + pad), float("nan"), dtype=K.dtype, device=K.device)
    Kp = buf[:, :, :N]
    Kp.copy_(K)
    Kp.masked_fill_(torch.ones(N, N, dtype=torch.bool, device=K.device).triu(1), float("nan"))
    assert bool(torch.isnan(Kp[:, 0, 1:]).all()) and (pad == 0) == Kp.is_contiguous()
    return Kp


@pytest.mark.parametrize("B,N,tables,pad,dtype", [(3, 257, True, 0, torch.float32), (8, 1280, True, 0, torch.float32),
                                                  (9, 640, False, 0, torch.float32), (3, 257, True, 37, torch.float32),
                                                  (4, 256, True, 0, torch.float64), (3, 640, False, 0, torch.float64)])
def test_potrf_reads_only_the_lower_triangle(ops, B, N, tables, pad, dtype):
    """include/volt_hip.h promises it for volt_potrf_k_f32 and volt_potrf_k_f64 (ops.potrf documents it): short series, the batched
    one launch, launch-per-column, a strided view with row stride N + 37; fp64 in one launch and launch-per-column.  Same bits
    as from the symmetric matrix -- except the fp64 launch-per-column path, whose K slices land through fp64 atomics in any
    order: there to fp64 round-off (the 1e-12 of test_null_workspace_is_the_launch_per_column_path)."""
    p = _problem("wishart", B, N, dtype)
    f = ops.potrf(p["K"], tables=tables)
    fp = ops.potrf(_poisoned(p["K"], pad), tables=tables)
    assert int(f.info.abs().sum()) == 0 and int(fp.info.abs().sum()) == 0, fp.info
    if dtype == torch.float64 and not tables:
        assert float((fp.L - f.L).abs().amax()) <= 1e-12 * float(f.L.abs().amax())       # (NaN fails this)
        assert float((fp.Winv - f.Winv).abs().amax()) <= 1e-9 * float(f.Winv.abs().amax())
    else:
        assert torch.equal(fp.L, f.L) and torch.equal(fp.Winv, f.Winv)


@pytest.mark.parametrize("B,N,tables,pad", [(3, 257, True, 0), (8, 1280, True, 0), (1, 385, True, 0), (9, 640, False, 0), (3, 257, True, 37)])
def test_mll_step_reads_only_the_lower_triangle(ops, B, N, tables, pad):
    """Without VOLT_REFINE_ALPHA the step reads what the factorisation reads (with it the header says BOTH triangles)."""
    p = _problem("wishart", B, N)
    out, alpha, info = ops.mll_step(p["K"], p["r"], p["s2"], tables=tables)
    assert int(info.abs().sum()) == 0
    out, alpha = out.clone(), alpha.clone()
    out_p, alpha_p, info_p = ops.mll_step(_poisoned(p["K"], pad), p["r"], p["s2"], tables=tables)
    assert int(info_p.abs().sum()) == 0, info_p
    assert torch.equal(out_p, out) and torch.equal(alpha_p, alpha)
