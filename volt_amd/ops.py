"""Tensor-level wrappers over the C ABI (device pointers in, torch tensors out).

Everything here requires CUDA(HIP) tensors; there is deliberately no CPU path.  PyTorch is used
for device memory and streams only.
"""
from __future__ import annotations

import torch

from . import _lib

TILE = 128


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.VoltHipError(
                "volt_amd ops need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")


def padded_n(n: int) -> int:
    return (n + TILE - 1) // TILE * TILE


def cumtrapz(y: torch.Tensor, x: torch.Tensor, square: bool = False) -> torch.Tensor:
    """CumTrapz (voltron/kernels/VolKernel.py:4-10).  y [..., N]; x [N] or y-shaped."""
    _need_gpu(y, x)
    if y.dtype not in (torch.float32, torch.float64):
        y = y.float()
    x = x.to(y.dtype)
    n = y.shape[-1]
    if x.shape[-1] != n:
        raise ValueError("x and y disagree on N")
    yb = y.reshape(-1, n).contiguous()
    B = yb.shape[0]
    if x.ndim == 1:
        xb, bsx = x.contiguous(), 0
    else:
        xb = x.expand(y.shape).reshape(-1, n).contiguous()
        bsx = n
    V = torch.empty_like(yb)
    fn = _lib.lib().volt_cumtrapz_f32 if y.dtype == torch.float32 else _lib.lib().volt_cumtrapz_f64
    _lib.check(fn(yb.data_ptr(), n, xb.data_ptr(), bsx, V.data_ptr(), B, n, int(square), _lib.stream_ptr()),
               "volt_cumtrapz")
    return V.reshape(y.shape)


def fill(V: torch.Tensor) -> torch.Tensor:
    """K[..., i, j] = V[..., min(i, j)] (voltron/kernels/VolKernel.py:30-33)."""
    _need_gpu(V)
    n = V.shape[-1]
    Vb = V.reshape(-1, n).contiguous()
    B = Vb.shape[0]
    K = torch.empty(B, n, n, dtype=V.dtype, device=V.device)
    fn = _lib.lib().volt_fill_f32 if V.dtype == torch.float32 else _lib.lib().volt_fill_f64
    _lib.check(fn(Vb.data_ptr(), K.data_ptr(), B, n, n, n * n, _lib.stream_ptr()), "volt_fill")
    return K.reshape(*V.shape[:-1], n, n)


_TAPS = {}


def ewma_weights(k: int, device) -> torch.Tensor:
    """The reference's taps, computed with the same torch expression (voltron/means/EWMA.py:21-24); cached per
    (k, device) -- the reference rebuilds them (and a Conv1d) on every call, here that would be a host-to-device
    copy per training iteration."""
    key = (int(k), str(device))
    if key not in _TAPS:
        alpha = 2. / (k + 1)
        wghts = alpha * (1 - alpha) ** (torch.arange(k - 1, -1, -1))
        _TAPS[key] = (wghts / wghts.sum()).to(torch.float32).to(device)
    return _TAPS[key]


def ewma(y: torch.Tensor, k: int) -> torch.Tensor:
    """EWMA(y, k) (voltron/means/EWMA.py:20-37): y [..., N] -> [..., N+1] fp32, on the device."""
    _need_gpu(y)
    n = y.shape[-1]
    yb = y.to(torch.float32).reshape(-1, n).contiguous()
    B = yb.shape[0]
    w = ewma_weights(k, y.device)
    out = torch.empty(B, n + 1, dtype=torch.float32, device=y.device)
    _lib.check(_lib.lib().volt_ewma_f32(yb.data_ptr(), n, w.data_ptr(), k, out.data_ptr(), B, n, _lib.stream_ptr()),
               "volt_ewma")
    return out.reshape(*y.shape[:-1], n + 1)


def info_internal(info: torch.Tensor) -> int:
    """How many entries of a factorisation's ``info`` report an INTERNAL error of the library (a hand-off time-out inside a
    one-launch step, a workspace that does not hold its tables: include/volt_hip.h) -- as opposed to a non-positive pivot
    (info > 0), the only thing gpytorch's jitter ladder is for.  One host read."""
    return int((info <= _lib.INFO_INTERNAL_MAX).sum().item())


class CholeskyFactor:
    """Result of `potrf`: padded factor A [B,Np,Np] (lower), inverse diagonal blocks, info [B]."""

    def __init__(self, A, Winv, info, n):
        self.A, self.Winv, self.info, self.n = A, Winv, info, n

    @property
    def L(self) -> torch.Tensor:
        return torch.tril(self.A[:, : self.n, : self.n])


def _scratch(nbytes: int, device, buf: torch.Tensor | None = None):
    """The one rule for scratch handed to the library: ``buf`` is nbytes + 256 bytes of uint8 and ``ptr`` the first
    256-byte-aligned address inside it.  Returns (buf, ptr); a ``buf`` made here earlier (the per-shape caches) is kept."""
    if buf is None:
        buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return buf, (buf.data_ptr() + 255) // 256 * 256


def _cached_scratch(cache: dict, key, nbytes: int, device):
    """Scratch kept in ``cache`` under ``key`` and reused across calls; calls that share a buffer are ordered by their
    stream.  Returns (aligned pointer, whether the buffer is new)."""
    fresh = key not in cache
    if fresh and len(cache) >= 8:                               # a handful of shapes is what a run has; drop the oldest
        cache.pop(next(iter(cache)))
    cache[key], ptr = _scratch(nbytes, device, cache.get(key))
    return ptr, fresh


_POTRF_WS = {}


def _potrf_workspace(B: int, Np: int, device):
    """Caller-owned scratch of volt_potrf_ws_f32, one buffer per (device, stream, B, Np), reused across calls -- the
    jitter ladder and the many small-matrix call sites would otherwise allocate up to 277 MB per call.  Returns
    (aligned pointer or None, bytes)."""
    nbytes = int(_lib.lib().volt_potrf_workspace_bytes(B, Np))
    if not nbytes:
        return None, 0
    ptr, fresh = _cached_scratch(_POTRF_WS, (device.index, _lib.stream_ptr(), B, Np), nbytes, device)
    if fresh:
        _lib.check(_lib.lib().volt_potrf_workspace_init_f32(ptr, nbytes, B, Np, _lib.stream_ptr()), "volt_potrf_workspace_init")
    return ptr, nbytes


def _potrf_ws_f64(B: int, Np: int, device):
    """The few KB of progress words the fp64 one-launch schedule wants (csrc/batch64_step.hip): one buffer per (device, stream,
    B, Np), as for the fp32 scratch.  Returns (aligned pointer or None, bytes)."""
    nbytes = int(_lib.lib().volt_potrf_workspace_bytes_f64(B, Np))
    if not nbytes:
        return None, 0
    return _cached_scratch(_POTRF_WS, (device.index, _lib.stream_ptr(), B, Np, "f64"), nbytes, device)[0], nbytes


def potrf_f64_inplace(A: torch.Tensor, Winv: torch.Tensor, info: torch.Tensor) -> None:
    """volt_potrf_ws_f64 on a prepared [B,Np,Np] fp64 buffer (the factor replaces it)."""
    B, Np = A.shape[0], A.shape[1]
    wp, nbytes = _potrf_ws_f64(B, Np, A.device)
    _lib.check(_lib.lib().volt_potrf_ws_f64(A.data_ptr(), Winv.data_ptr(), info.data_ptr(), B, Np, wp, nbytes, _lib.stream_ptr()),
               "volt_potrf")


def potrf(K: torch.Tensor, sigma2: torch.Tensor | None = None, jitter: float = 0.0, tables: bool = True) -> CholeskyFactor:
    """Batched Cholesky of K + (sigma2 + jitter) I.  K [B,N,N] fp32 or fp64 (only the lower triangle is read); the
    factor keeps K's dtype (fp32: volt_potrf_f32 on v_mfma_f32_32x32x2; fp64: volt_potrf_f64 on v_mfma_f64_16x16x4).
    ``tables=False``: the launch-per-column schedules only (no scratch handed over, so no one-launch step) -- what the
    wrappers fall back to when a one-launch step reports an internal error (`info_internal`)."""
    _need_gpu(K, sigma2)
    if K.dtype not in (torch.float32, torch.float64) or K.ndim != 3:
        raise ValueError("potrf expects a [B,N,N] fp32 or fp64 tensor")
    if K.stride(-1) != 1:
        K = K.contiguous()
    B, n, _ = K.shape
    Np = padded_n(n)
    A = torch.empty(B, Np, Np, dtype=K.dtype, device=K.device)
    Winv = torch.empty(B, Np // TILE, TILE, TILE, dtype=K.dtype, device=K.device)
    info = torch.empty(B, dtype=torch.int32, device=K.device)
    s2 = None
    if sigma2 is not None:
        s2 = sigma2.to(K.dtype).expand(B).contiguous()
    L = _lib.lib()
    st = _lib.stream_ptr()
    s2p = s2.data_ptr() if s2 is not None else None
    if K.dtype == torch.float32:
        # straight from K (no copy-in pass); scratch for the small-batch schedules (0 bytes above 64 matrices and below
        # 3 block columns)
        wp, nbytes = _potrf_workspace(B, Np, K.device) if tables else (None, 0)
        _lib.check(L.volt_potrf_k_f32(K.data_ptr(), K.stride(1), K.stride(0), s2p, float(jitter), A.data_ptr(),
                                      Winv.data_ptr(), info.data_ptr(), B, n, wp, nbytes,
                                      _lib.WS_INITIALISED if wp else 0, st), "volt_potrf_k")
    else:
        # straight from K where the shape runs as one launch (small / medium batches); prepare + launch-per-column otherwise
        wp, nbytes = _potrf_ws_f64(B, Np, K.device) if tables else (None, 0)
        _lib.check(L.volt_potrf_k_f64(K.data_ptr(), K.stride(1), K.stride(0), s2p, float(jitter), A.data_ptr(), Winv.data_ptr(),
                                      info.data_ptr(), B, n, wp, nbytes, st), "volt_potrf_k")
    return CholeskyFactor(A, Winv, info, n)


def _pad_rhs(f: CholeskyFactor, rhs: torch.Tensor) -> torch.Tensor:
    B, Np = f.A.shape[0], f.A.shape[1]
    out = torch.zeros(B, Np, dtype=f.A.dtype, device=f.A.device)
    out[:, : f.n] = rhs.reshape(B, f.n)
    return out


def trsv(f: CholeskyFactor, rhs: torch.Tensor, transpose: bool = False, check: bool = False) -> torch.Tensor:
    """L^-1 rhs (or L^-T rhs) in the factor's dtype.  rhs [B,N] -> [B,N].  One launch (csrc/trsv.hip).
    ``check`` reads the solve's error word back (a device synchronisation) and raises if a hand-off timed out --
    without it a time-out is visible only as NaN in the result."""
    _need_gpu(rhs)
    r = _pad_rhs(f, rhs)
    out = torch.empty_like(r)
    scratch = torch.empty_like(r)
    B, Np = r.shape
    L = _lib.lib()
    if f.A.dtype == torch.float32:
        fn = L.volt_trsv_lower_t_f32 if transpose else L.volt_trsv_lower_f32
    else:
        fn = L.volt_trsv_lower_t_f64 if transpose else L.volt_trsv_lower_f64
    _lib.check(fn(f.A.data_ptr(), f.Winv.data_ptr(), r.data_ptr(), out.data_ptr(), scratch.data_ptr(), B, Np,
                  _lib.stream_ptr()), "volt_trsv")
    if check and int(scratch.view(torch.int32).reshape(-1)[1].item()) != 0:
        raise _lib.VoltHipError("volt_trsv: a block hand-off timed out (the result holds NaN blocks)")
    return out[:, : f.n]


def cholesky_solve(f: CholeskyFactor, rhs: torch.Tensor) -> torch.Tensor:
    """(L L^T)^-1 rhs for one right-hand side per matrix (torch.cholesky_solve, rollout_utils.py:36)."""
    return trsv(f, trsv(f, rhs), transpose=True)


def trtri(f: CholeskyFactor) -> torch.Tensor:
    """Y = L^-T as an upper-triangular [B,N,N] tensor in the factor's dtype (volt_trtri_f32 / volt_trtri_f64)."""
    B, Np = f.A.shape[0], f.A.shape[1]
    Y = torch.empty(B, Np, Np, dtype=f.A.dtype, device=f.A.device)
    L = _lib.lib()
    if f.A.dtype == torch.float32:
        _lib.check(L.volt_trtri_f32(f.A.data_ptr(), f.Winv.data_ptr(), Y.data_ptr(), B, Np, _lib.stream_ptr()), "volt_trtri")
    else:
        # a few KB of progress words let the whole inverse run as one launch (csrc/batch64_step.hip); 0 bytes: launch per row
        nbytes = int(L.volt_trtri_workspace_bytes_f64(B, Np))
        ws, wp = _scratch(nbytes, f.A.device) if nbytes else (None, None)
        _lib.check(L.volt_trtri_ws_f64(f.A.data_ptr(), f.Winv.data_ptr(), Y.data_ptr(), B, Np, wp, nbytes, _lib.stream_ptr()), "volt_trtri")
    return torch.triu(Y[:, : f.n, : f.n])


def cached_workspace(holder, attr: str, cls, *shape):
    """``holder.<attr>`` if it ``fits(*shape)`` -- the constructor's own arguments, the device among them --, else a new
    ``cls(*shape)`` kept there: how the MLL and ELBO objects carry one workspace of each kind from iteration to iteration."""
    ws = getattr(holder, attr, None)
    if ws is None or not ws.fits(*shape):
        ws = cls(*shape)
        setattr(holder, attr, ws)
    return ws


class MllWorkspace:
    """Caller-owned scratch for volt_mll_step_f32 / _f64, reusable across steps of the same (B, N, dtype)."""

    def __init__(self, B: int, N: int, want_grad: bool, device, dtype=torch.float32):
        self.B, self.N, self.want_grad, self.dtype = B, N, bool(want_grad), dtype
        L = _lib.lib()
        query = L.volt_mll_workspace_bytes if dtype == torch.float32 else L.volt_mll_workspace_bytes_f64
        nbytes = query(B, N, int(want_grad))
        self.buf, self.ptr = _scratch(nbytes, device)
        self.flags = int(bool(want_grad)) * _lib.WANT_GRAD
        if dtype == torch.float32:                      # the launch-schedule table of this shape, once (mid-size batches)
            with torch.cuda.device(self.buf.device):
                _lib.check(L.volt_mll_workspace_init_f32(self.ptr, B, N, int(want_grad), _lib.stream_ptr()), "volt_mll_workspace_init")
            self.flags |= _lib.WS_INITIALISED           # ... and the step is told so (the library keeps no record of it)
        self.out = torch.empty(B, 8, dtype=dtype, device=device)
        self.alpha = torch.empty(B, N, dtype=dtype, device=device)
        self.info = torch.empty(B, dtype=torch.int32, device=device)

    def fits(self, B, N, want_grad, device, dtype=torch.float32):
        return ((self.B, self.N, self.want_grad, self.buf.device, self.dtype) == (B, N, bool(want_grad), device, dtype))


def mll_step(K: torch.Tensor, resid: torch.Tensor, sigma2: torch.Tensor, ws: MllWorkspace | None = None,
             want_grad: bool = True, jitter: float = 0.0, refine_alpha: bool = False, tables: bool = True):
    """One MLL(+grad) evaluation with K resident, in K's dtype: fp32 -> volt_mll_step_f32 (v_mfma_f32_32x32x2), fp64 ->
    volt_mll_step_f64 (v_mfma_f64_16x16x4).  Returns (out [B,8], alpha [B,N], info [B]); see include/volt_hip.h for the
    meaning of out's columns.  ``refine_alpha`` (fp32, with want_grad; opt-in): one step of iterative refinement of alpha
    against K itself (VOLT_REFINE_ALPHA) -- both triangles of K must hold the symmetric matrix.
    ``tables=False`` (fp32): the workspace is NOT declared initialised, so the step runs the table-free launch-per-column
    schedules -- the fallback of the wrappers when a one-launch step reports an internal error (`info_internal`)."""
    _need_gpu(K, resid, sigma2)
    if K.ndim != 3 or K.dtype not in (torch.float32, torch.float64):
        raise ValueError("K must be [B,N,N] fp32 or fp64")
    dt = K.dtype
    B, n, _ = K.shape
    if K.stride(-1) != 1:
        K = K.contiguous()
    resid = resid.reshape(B, n).to(dt).contiguous()
    s2 = sigma2.to(dt).expand(B).contiguous()
    if ws is None or not ws.fits(B, n, want_grad, K.device, dt):
        ws = MllWorkspace(B, n, want_grad, K.device, dt)
    fn = _lib.lib().volt_mll_step_f32 if dt == torch.float32 else _lib.lib().volt_mll_step_f64
    _lib.check(fn(K.data_ptr(), K.stride(1), K.stride(0), resid.data_ptr(), s2.data_ptr(), float(jitter), ws.out.data_ptr(),
                  ws.alpha.data_ptr(), ws.info.data_ptr(), ws.ptr, B, n,
                  ((ws.flags if tables else ws.flags & ~_lib.WS_INITIALISED) | (_lib.REFINE_ALPHA if (refine_alpha and want_grad) else 0))
                  if dt == torch.float32 else int(want_grad),
                  _lib.stream_ptr()), "volt_mll_step")
    return ws.out, ws.alpha, ws.info


# ------------------------------------------------------------------ linear-time Brownian-motion solver (csrc/bm.hip)
class BmWorkspace:
    """Caller-owned scratch and outputs of volt_bm_step_* / volt_bm_solve_*, reusable across calls of the same
    (B, N, H, dtype): (1 + H) B N doubles, nothing O(N^2).  H = 0: the step alone (out, alpha); H >= 1 adds X [B,N,H]."""

    def __init__(self, B: int, N: int, device, dtype=torch.float32, H: int = 0):
        self.B, self.N, self.H, self.dtype = B, N, H, dtype
        nbytes = int(_lib.lib().volt_bm_workspace_bytes(B, N, max(H, 1)))
        self.buf, self.ptr = _scratch(nbytes, device)
        self.info = torch.empty(B, dtype=torch.int32, device=device)
        if H == 0:
            self.out = torch.empty(B, 8, dtype=dtype, device=device)
            self.alpha = torch.empty(B, N, dtype=dtype, device=device)
        else:
            self.X = torch.empty(B, N, H, dtype=dtype, device=device)

    def fits(self, B, N, device, dtype=torch.float32, H=0):
        return (self.B, self.N, self.buf.device, self.dtype, self.H) == (B, N, device, dtype, H)


def _bm_args(x, vol, sigma2, B, dt):
    if x.ndim != 1:
        raise ValueError("the Brownian-motion grid x must be 1-D [N], shared by the batch")
    return x.to(dt).contiguous(), vol.to(dt).reshape(-1).expand(B).contiguous(), sigma2.to(dt).reshape(-1).expand(B).contiguous()


def bm_step(x: torch.Tensor, vol: torch.Tensor, sigma2: torch.Tensor, resid: torch.Tensor, ws: BmWorkspace | None = None,
            want_grad: bool = True):
    """One MLL(+grad) evaluation of the Brownian-motion prior K = vol * min(x, x') + sigma2 I in O(N) (volt_bm_step_f32 /
    _f64 by resid's dtype; the arithmetic is fp64 either way).  x [N] (0 <= x_0 < x_1 < ..), vol [B], sigma2 [B],
    resid [B,N].  Returns (out [B,8], alpha [B,N], info [B]) with the meaning of `mll_step`'s; they live in ``ws``."""
    _need_gpu(x, vol, sigma2, resid)
    dt = torch.float64 if resid.dtype == torch.float64 else torch.float32
    if resid.ndim != 2:
        raise ValueError("resid must be [B,N]")
    B, n = resid.shape
    if x.shape[-1] != n:
        raise ValueError("x and resid disagree on N")
    x, vol, sigma2 = _bm_args(x, vol, sigma2, B, dt)
    return _chain_step("volt_bm_step", (x.data_ptr(), vol.data_ptr()), sigma2, resid, dt, ws, want_grad)


def vk_step(V: torch.Tensor, sigma2: torch.Tensor, resid: torch.Tensor, ws: BmWorkspace | None = None, want_grad: bool = True):
    """One MLL(+grad) evaluation of the volatility-kernel data model K_b = V_b[min(i, j)] + sigma2_b I in O(N) (volt_vk_step_f32 /
    _f64 by resid's dtype; the arithmetic is fp64 either way), without K.  V [N] (one grid for all series) or [B,N] (each
    series its own: non-decreasing rows, V_0 >= 0 -- what `cumtrapz(vol, x, square=True)` returns), sigma2 [B] (or one
    value), resid [B,N].  Returns (out [B,8], alpha [B,N], info [B]) with the meaning of `mll_step`'s; they live in ``ws``."""
    _need_gpu(V, sigma2, resid)
    dt = torch.float64 if resid.dtype == torch.float64 else torch.float32
    if resid.ndim != 2:
        raise ValueError("resid must be [B,N]")
    B, n = resid.shape
    V, bsv = _vk_grid(V, B, n, dt)
    sigma2 = sigma2.to(dt).reshape(-1).expand(B).contiguous()
    return _chain_step("volt_vk_step", (V.data_ptr(), bsv), sigma2, resid, dt, ws, want_grad)


def _vk_grid(V, B, n, dt):
    """V [N] or [B,N] as volt_vk_* take it: (V in ``dt`` with unit inner stride and rows that do not overlap, bsv)."""
    if V.ndim not in (1, 2) or V.shape[-1] != n:
        raise ValueError("V must be [N] or [B,N] with resid's N")
    if V.ndim == 2 and V.shape[0] != B:
        raise ValueError("V [B,N] and resid disagree on B")
    V = V.to(dt)
    if V.stride(-1) != 1 or (V.ndim == 2 and B > 1 and V.stride(0) < n):
        V = V.contiguous()
    return V, (0 if V.ndim == 1 or B == 1 else V.stride(0))


def vk_forms(V: torch.Tensor, jitter, resid: torch.Tensor):
    """The conditioning scalars of a forecast from the volatility-kernel data model in O(N) (volt_vk_forms_f32 / _f64 by
    resid's dtype; the arithmetic and the outputs are fp64 either way): per series, with A_b = V_b[min(i, j)] + jitter_b I,
    out[b] = (V'A^-1 V, V'A^-1 r, r'A^-1 r, logdet A).  V [N] or [B,N] (strided rows allowed) as for `vk_step`; jitter a
    number or [B], >= 0 (0 is legal); resid [B,N].  Returns (out [B,4] fp64, info [B] int32), freshly allocated."""
    _need_gpu(V, resid, jitter if torch.is_tensor(jitter) else None)
    dt = torch.float64 if resid.dtype == torch.float64 else torch.float32
    if resid.ndim != 2:
        raise ValueError("resid must be [B,N]")
    B, n = resid.shape
    V, bsv = _vk_grid(V, B, n, dt)
    resid = resid.to(dt).contiguous()
    jit = torch.as_tensor(jitter, dtype=torch.float64, device=resid.device).reshape(-1).expand(B).contiguous()
    out = torch.empty(B, 4, dtype=torch.float64, device=resid.device)
    info = torch.empty(B, dtype=torch.int32, device=resid.device)
    fn = _lib.lib().volt_vk_forms_f32 if dt == torch.float32 else _lib.lib().volt_vk_forms_f64
    with torch.cuda.device(resid.device):
        _lib.check(fn(V.data_ptr(), bsv, jit.data_ptr(), resid.data_ptr(), out.data_ptr(), info.data_ptr(), B, n,
                      _lib.stream_ptr()), "volt_vk_forms")
    return out, info


def _chain_step(entry, grid_args, sigma2, resid, dt, ws, want_grad):
    """What `bm_step` and `vk_step` share once their own arguments are checked and marshalled: the residual, the workspace
    and the call of ``entry``_f32 / _f64, whose leading arguments ``grid_args`` are all the two entries differ in."""
    B, n = resid.shape
    resid = resid.to(dt).contiguous()
    if ws is None or not ws.fits(B, n, resid.device, dt):
        ws = BmWorkspace(B, n, resid.device, dt)
    fn = getattr(_lib.lib(), entry + ("_f32" if dt == torch.float32 else "_f64"))
    with torch.cuda.device(resid.device):
        _lib.check(fn(*grid_args, sigma2.data_ptr(), resid.data_ptr(), ws.out.data_ptr(), ws.alpha.data_ptr(),
                      ws.info.data_ptr(), ws.ptr, B, n, _lib.WANT_GRAD if want_grad else 0, _lib.stream_ptr()), entry)
    return ws.out, ws.alpha, ws.info


def bm_post(x: torch.Tensor, xs_sorted: torch.Tensor, vol: torch.Tensor, sigma2: torch.Tensor, resid: torch.Tensor):
    """The forms of the Brownian-motion posterior at H test points in ONE O(N H) sweep with no workspace (volt_bm_post_f32 /
    _f64 by resid's dtype; the arithmetic and the outputs are fp64 either way): per series, with A_b = vol_b min(x, x') +
    sigma2_b I and k_h = vol_b min(x, xi_h), out[b] = rows (k_h'A^-1 r, k_h'A^-1 k_h, k_h'A^-1 k_{h+1}).  x [N] (one grid for
    all series) or [B,N] (strided rows allowed); xs_sorted [H] ascending, >= 0, shared; vol, sigma2 [B] (or one value);
    resid [B,N].  Returns (out [B,3,H] fp64, info [B] int32), freshly allocated; info[b] = i + 1 at the first bad pivot,
    -(h + 1) at the first test point that is NaN / inf, negative or out of order, and the series' rows are then NaN."""
    _need_gpu(x, xs_sorted, vol, sigma2, resid)
    dt = torch.float64 if resid.dtype == torch.float64 else torch.float32
    if resid.ndim != 2:
        raise ValueError("resid must be [B,N]")
    if xs_sorted.ndim != 1 or xs_sorted.shape[0] < 1:
        raise ValueError("xs_sorted must be [H], H >= 1")
    B, n = resid.shape
    if x.ndim not in (1, 2) or x.shape[-1] != n:
        raise ValueError("x must be [N] or [B,N] with resid's N")
    if x.ndim == 2 and x.shape[0] != B:
        raise ValueError("x [B,N] and resid disagree on B")
    x, bsx = _vk_grid(x, B, n, dt)
    H = xs_sorted.shape[0]
    xs = xs_sorted.to(dt).contiguous()
    vol = vol.to(dt).reshape(-1).expand(B).contiguous()
    sigma2 = sigma2.to(dt).reshape(-1).expand(B).contiguous()
    resid = resid.to(dt).contiguous()
    out = torch.empty(B, 3, H, dtype=torch.float64, device=resid.device)
    info = torch.empty(B, dtype=torch.int32, device=resid.device)
    fn = _lib.lib().volt_bm_post_f32 if dt == torch.float32 else _lib.lib().volt_bm_post_f64
    with torch.cuda.device(resid.device):
        _lib.check(fn(x.data_ptr(), bsx, xs.data_ptr(), vol.data_ptr(), sigma2.data_ptr(), resid.data_ptr(), out.data_ptr(),
                      info.data_ptr(), B, n, H, _lib.stream_ptr()), "volt_bm_post")
    return out, info


def _draw_buffers(z, out, info, info_shape):
    """The output pair of the chain draws: the caller's ``out`` / ``info`` (contiguous, z's shape and dtype / int32) or fresh ones."""
    if out is None:
        out = torch.empty_like(z)
    elif out.shape != z.shape or out.dtype != z.dtype or not out.is_contiguous() or out.device != z.device:
        raise ValueError("out must be contiguous with z's shape, dtype and device")
    if info is None:
        info = torch.empty(info_shape, dtype=torch.int32, device=z.device)
    elif tuple(info.shape) != tuple(info_shape) or info.dtype != torch.int32 or not info.is_contiguous() or info.device != z.device:
        raise ValueError(f"info must be a contiguous int32 tensor of shape {tuple(info_shape)} on z's device")
    return out, info


def _per_series(v, G, device):
    return torch.as_tensor(v, dtype=torch.float64, device=device).reshape(-1).expand(G).contiguous()


def markov_draw(mean: torch.Tensor, diag: torch.Tensor, off: torch.Tensor, z: torch.Tensor, jitter=0.0, exp: bool = False,
                out: torch.Tensor | None = None, info: torch.Tensor | None = None):
    """mean + chol(C + jitter I) z in O(S H) for the Markov covariance C = gp._markov_cov(diag, off), never formed
    (volt_markov_draw_f32 / _f64 by z's dtype; fp64 arithmetic either way).  mean, diag, off [G,H] (the last entry of
    off is not read); z [G,S,H]; jitter a number or [G], >= 0; ``exp``: the exponential of the draw, computed in double and
    rounded once.  Strided inputs are accepted (copied where the kernel needs them dense).  Returns (out [G,S,H] in z's dtype,
    info [G] int32) -- ``out`` / ``info`` given: written in place.  info[g] = i + 1 at the first step whose pivot is not a
    positive finite number; the series' outputs are then all NaN."""
    _need_gpu(mean, diag, off, z, jitter if torch.is_tensor(jitter) else None)
    if z.ndim != 3:
        raise ValueError("z must be [G,S,H]")
    G, S, H = z.shape
    if G < 1 or S < 1 or H < 1:
        raise ValueError("z [G,S,H] must not be empty")
    for name, t in (("mean", mean), ("diag", diag), ("off", off)):
        if tuple(t.shape) != (G, H):
            raise ValueError(f"{name} must be [G,H] = {(G, H)}, got {tuple(t.shape)}")
    dt = torch.float64 if z.dtype == torch.float64 else torch.float32
    z = z.to(dt).contiguous()
    mean, diag, off = (t.to(torch.float64).contiguous() for t in (mean, diag, off))
    jit = _per_series(jitter, G, z.device)
    out, info = _draw_buffers(z, out, info, (G,))
    fn = _lib.lib().volt_markov_draw_f32 if dt == torch.float32 else _lib.lib().volt_markov_draw_f64
    with torch.cuda.device(z.device):
        _lib.check(fn(mean.data_ptr(), diag.data_ptr(), off.data_ptr(), z.data_ptr(), jit.data_ptr(), out.data_ptr(),
                      info.data_ptr(), G, S, H, _lib.DRAW_EXP if exp else 0, _lib.stream_ptr()), "volt_markov_draw")
    return out, info


def markov_mix(lz: torch.Tensor, V: torch.Tensor, mean: torch.Tensor) -> torch.Tensor:
    """mean + (L_j z_j)_j V' of a MultitaskBMGP(posterior="chain") draw (volt_markov_mix_f32): lz [T,S,n] fp64 (ops.markov_draw
    with G = T), V [T,T], mean [n,T].  The sum over the T directions is fp64 in a fixed order, rounded once.  Returns [S,n,T] fp32."""
    _need_gpu(lz, V, mean)
    if lz.ndim != 3 or lz.dtype != torch.float64:
        raise ValueError("lz must be [T,S,n] float64")
    T, S, n = lz.shape
    if tuple(V.shape) != (T, T) or tuple(mean.shape) != (n, T):
        raise ValueError(f"V must be [T,T] = {(T, T)} and mean [n,T] = {(n, T)}, got {tuple(V.shape)} and {tuple(mean.shape)}")
    lz, V, mean = lz.contiguous(), V.to(torch.float64).contiguous(), mean.to(torch.float32).contiguous()
    out = torch.empty(S, n, T, dtype=torch.float32, device=lz.device)
    with torch.cuda.device(lz.device):
        _lib.check(_lib.lib().volt_markov_mix_f32(lz.data_ptr(), V.data_ptr(), mean.data_ptr(), out.data_ptr(), T, S, n,
                                                  _lib.stream_ptr()), "volt_markov_mix")
    return out


def vk_draw(pred_vol: torch.Tensor, vol_last, vlr, dx, mean: torch.Tensor, z: torch.Tensor, jitter=0.0, reps: int = 1,
            out: torch.Tensor | None = None, info: torch.Tensor | None = None):
    """The joint draw over H appended points from the volatility-kernel data model in O(S H) (volt_vk_draw_f32 / _f64 by z's
    dtype; fp64 arithmetic either way): mean + chol(W[min(s,t)] + jitter I) z with W_h = vlr + the CumTrapz of
    [vol_last, pred_vol]^2 over a uniform step dx less its first entry, formed on the fly.  pred_vol [G,S,H]; vol_last, vlr
    (= V_last - rho), dx, jitter numbers or [G]; mean [G,H]; z [G,S*reps,H]: ``reps`` consecutive paths share a row of
    pred_vol.  Returns (out like z, info [G,S] int32; ``out`` / ``info`` given: written in place); info = i + 1 at the first
    failed pivot of a pred_vol row, whose paths are then all NaN."""
    _need_gpu(pred_vol, mean, z, *(t for t in (vol_last, vlr, dx, jitter) if torch.is_tensor(t)))
    if pred_vol.ndim != 3 or z.ndim != 3:
        raise ValueError("pred_vol must be [G,S,H] and z [G,S*reps,H]")
    G, S, H = pred_vol.shape
    if G < 1 or S < 1 or H < 1 or reps < 1:
        raise ValueError("pred_vol [G,S,H] must not be empty and reps >= 1")
    if tuple(z.shape) != (G, S * reps, H):
        raise ValueError(f"z must be [G,S*reps,H] = {(G, S * reps, H)}, got {tuple(z.shape)}")
    if tuple(mean.shape) != (G, H):
        raise ValueError(f"mean must be [G,H] = {(G, H)}, got {tuple(mean.shape)}")
    dt = torch.float64 if z.dtype == torch.float64 else torch.float32
    z = z.to(dt).contiguous()
    pred_vol = pred_vol.to(dt).contiguous()
    mean = mean.to(torch.float64).contiguous()
    vol_last, vlr, dx, jit = (_per_series(t, G, z.device) for t in (vol_last, vlr, dx, jitter))
    out, info = _draw_buffers(z, out, info, (G, S))
    fn = _lib.lib().volt_vk_draw_f32 if dt == torch.float32 else _lib.lib().volt_vk_draw_f64
    with torch.cuda.device(z.device):
        _lib.check(fn(pred_vol.data_ptr(), vol_last.data_ptr(), vlr.data_ptr(), dx.data_ptr(), mean.data_ptr(), z.data_ptr(),
                      jit.data_ptr(), out.data_ptr(), info.data_ptr(), G, S, H, reps, _lib.stream_ptr()), "volt_vk_draw")
    return out, info


def bm_solve(x: torch.Tensor, vol: torch.Tensor, sigma2: torch.Tensor, R: torch.Tensor, ws: BmWorkspace | None = None):
    """X = (vol_b min(x, x') + sigma2_b I)^-1 R_b in O(N H) per series (volt_bm_solve_f32 / _f64 by R's dtype).
    R [B,N,H].  Returns (X [B,N,H], info [B]); they live in ``ws``."""
    _need_gpu(x, vol, sigma2, R)
    dt = torch.float64 if R.dtype == torch.float64 else torch.float32
    if R.ndim != 3:
        raise ValueError("R must be [B,N,H]")
    B, n, H = R.shape
    if x.shape[-1] != n:
        raise ValueError("x and R disagree on N")
    x, vol, sigma2 = _bm_args(x, vol, sigma2, B, dt)
    R = R.to(dt).contiguous()
    if ws is None or not ws.fits(B, n, R.device, dt, H):
        ws = BmWorkspace(B, n, R.device, dt, H)
    fn = _lib.lib().volt_bm_solve_f32 if dt == torch.float32 else _lib.lib().volt_bm_solve_f64
    with torch.cuda.device(R.device):
        _lib.check(fn(x.data_ptr(), vol.data_ptr(), sigma2.data_ptr(), R.data_ptr(), ws.X.data_ptr(), ws.info.data_ptr(), ws.ptr,
                      B, n, H, _lib.stream_ptr()), "volt_bm_solve")
    return ws.X, ws.info


# ------------------------------------------------------------------ GPCV stage
def gemm_nt(A: torch.Tensor, B: torch.Tensor, uplo_a: int = 0, uplo_b: int = 0) -> torch.Tensor:
    """A @ B.mT on the library's fp32 MFMA GEMM.  A [T,M,K], B [T,N,K] (or 2-D); uplo_* = 1 / 2 declare an
    operand lower / upper triangular so its zero 128-blocks are skipped.  Operands are zero-padded to the
    128 tile here (plumbing); the arithmetic is volt_gemm_nt_f32."""
    _need_gpu(A, B)
    two_d = A.ndim == 2
    A3 = (A.unsqueeze(0) if two_d else A).to(torch.float32)
    B3 = (B.unsqueeze(0) if B.ndim == 2 else B).to(torch.float32)
    T, M, K = A3.shape
    N = B3.shape[1]
    if B3.shape[0] != T or B3.shape[2] != K:
        raise ValueError("gemm_nt: A [T,M,K] and B [T,N,K] disagree")
    Mp, Np_, Kp = padded_n(M), padded_n(N), padded_n(K)
    Ap = torch.zeros(T, Mp, Kp, dtype=torch.float32, device=A.device)
    Bp = torch.zeros(T, Np_, Kp, dtype=torch.float32, device=A.device)
    Ap[:, :M, :K] = A3
    Bp[:, :N, :K] = B3
    Cp = torch.empty(T, Mp, Np_, dtype=torch.float32, device=A.device)
    _lib.check(_lib.lib().volt_gemm_nt_f32(Ap.data_ptr(), Kp, Mp * Kp, uplo_a, Bp.data_ptr(), Kp, Np_ * Kp, uplo_b,
                                           Cp.data_ptr(), Np_, Mp * Np_, 0, 1.0, 0.0, T, Mp, Np_, Kp,
                                           _lib.stream_ptr()), "volt_gemm_nt")
    C = Cp[:, :M, :N]
    return C[0] if two_d else C


GPCV_CV_K_MAX = 8                   # include/volt_hip.h: VOLT_GPCV_CV_K_MAX, volt_gpcv_cv_step_f32 takes 1 <= Kc <= 8 warp terms


def _f32(t, shape):
    return t.detach().reshape(shape).to(torch.float32).contiguous()


def _quad_args(gh_x, gh_w, min_var, min_scale, w_ell, w_kl):
    """The Gauss-Hermite table as the steps read it and the argument run every GPCV entry takes after its prior.  Returns
    (gh_x, gh_w, run): the caller holds the two tensors until its launch is queued."""
    gh_x, gh_w = gh_x.to(torch.float32).contiguous(), gh_w.to(torch.float32).contiguous()
    return gh_x, gh_w, (gh_x.data_ptr(), gh_w.data_ptr(), gh_x.numel(), float(min_var), float(min_scale), float(w_ell),
                        float(w_kl))


def _abc_arg(abc, lead, letter, reject=None):
    """The "cv" likelihood's abc checked as [lead,3,Kc] (``letter`` names ``lead`` in the message) and made fp32 contiguous.
    Returns (abc, Kc, whether a workspace can be sized); no abc: (None, 0, True).
    An out-of-range Kc is behaviour and differs by family.  ``reject`` None (the single-task steps): no workspace can be sized, so
    the caller passes none and the C entry returns its argument code ("invalid argument ...", pinned by
    tests/test_gpu_gpcv_cv.py).  ``reject`` a step's name (the multi-task step): VoltHipError from here."""
    if abc is None:
        return None, 0, True
    if abc.ndim != 3 or abc.shape[0] != lead or abc.shape[1] != 3:
        raise ValueError(f"abc must be [{letter},3,Kc]")
    Kc = abc.shape[2]
    ok = 1 <= Kc <= GPCV_CV_K_MAX
    if not ok and reject is not None:
        raise _lib.VoltHipError(f"{reject} takes 1 <= Kc <= {GPCV_CV_K_MAX} warp terms (got Kc = {Kc})")
    return _f32(abc, (lead, 3, Kc)), Kc, ok


def _step_workspace(cls, ws, sizeable, *key):
    """``ws`` if it fits ``key``, else a new ``cls(*key)``; None where ``_abc_arg`` found nothing to size one for."""
    if not sizeable:
        return None
    return ws if ws is not None and ws.fits(*key) else cls(*key)


def _ptrs(ws, *names):
    """The addresses of the workspace's ``names`` in that order; None for an output it does not have, or without a workspace."""
    vals = (getattr(ws, name) if ws is not None else None for name in names)
    return tuple(v.data_ptr() if torch.is_tensor(v) else v for v in vals)


class _GpcvStepWorkspace:
    """What the GPCV workspaces share: the scratch, the MLL workspace some of them begin with, the fp32 outputs, ``info``
    and ``fits``.  A subclass states its constructor key, its byte count and its outputs; the names it sets are its own."""
    _STEP = 'the "cv" GPCV step'

    def _checked_kc(self, Kc):
        if Kc < 0 or Kc > GPCV_CV_K_MAX:
            raise _lib.VoltHipError(f"{self._STEP} takes 1 <= Kc <= {GPCV_CV_K_MAX} warp terms (got Kc = {Kc})")
        return int(Kc)

    def _allocate(self, key, device, nbytes, outputs, n_info, mll_init=None):
        """``key``: the constructor's arguments without the device (what ``fits`` compares); ``outputs``: name -> shape, None
        for an output this workspace does not have; ``mll_init``: (B, N) of the MLL workspace the scratch begins with."""
        self._key, self.nbytes = key, int(nbytes)
        self.buf, self.ptr = _scratch(self.nbytes, device)
        if mll_init is not None:                         # the launch-schedule table of that step
            with torch.cuda.device(self.buf.device):
                _lib.check(_lib.lib().volt_mll_workspace_init_f32(self.ptr, *mll_init, 1, _lib.stream_ptr()),
                           "volt_mll_workspace_init")
        for name, shape in outputs.items():
            setattr(self, name, None if shape is None else torch.empty(shape, dtype=torch.float32, device=device))
        self.info = torch.empty(n_info, dtype=torch.int32, device=device)

    def _fits(self, device, *key):
        return (self.buf.device, *self._key) == (device, *key)


class GpcvWorkspace(_GpcvStepWorkspace):
    """Caller-owned scratch and outputs of volt_gpcv_step_f32, reusable across steps of the same (B,N).
    Kc > 0: the workspace of volt_gpcv_cv_step_f32 for Kc warp terms (adds .grad_abc [B,3,Kc])."""

    def __init__(self, B: int, N: int, want_dk: bool, device, Kc: int = 0):
        self.B, self.N, self.want_dk, self.Kc = B, N, bool(want_dk), self._checked_kc(Kc)
        L = _lib.lib()
        nbytes = L.volt_gpcv_cv_workspace_bytes(B, N, int(want_dk), self.Kc) if Kc else L.volt_gpcv_workspace_bytes(B, N, int(want_dk))
        self._allocate((B, N, self.want_dk, self.Kc), device, nbytes, mll_init=(B, N), n_info=B, outputs={
            "out": (B, 12), "grad_m": (B, N), "grad_mu": (B, N), "grad_Lq": (B, N, N),
            "grad_K": (B, N, N) if want_dk else None, "grad_abc": (B, 3, Kc) if Kc else None})

    def fits(self, B, N, want_dk, device, Kc=0):
        return self._fits(device, B, N, bool(want_dk), Kc)


def gpcv_step(K, resid, m, Lq, y, gh_x, gh_w, ws: GpcvWorkspace | None = None, want_dk: bool = False,
              jitter: float = 1e-3, min_var: float = 1e-6, min_scale: float = 1e-3, w_ell: float = 1.0,
              w_kl: float = 1.0):
    """One ELBO + gradient evaluation of the GPCV variational GP (include/volt_hip.h, volt_gpcv_step_f32).
    K [B,N,N] prior covariance without jitter; resid = m - prior mean, m, y [B,N]; Lq [B,N,N].
    Gradients are those of F = w_ell * ell - w_kl * KL (out[:, 9]).
    Returns the workspace: .out [B,12], .grad_m, .grad_mu, .grad_Lq (.grad_K if want_dk), .info."""
    return _gpcv_dense_step(K, resid, m, Lq, y, None, gh_x, gh_w, ws, want_dk, jitter, min_var, min_scale, w_ell, w_kl)


def gpcv_cv_step(K, resid, m, Lq, y, abc, gh_x, gh_w, ws: GpcvWorkspace | None = None, want_dk: bool = False,
                 jitter: float = 1e-3, min_var: float = 1e-6, min_scale: float = 1e-3, w_ell: float = 1.0,
                 w_kl: float = 1.0):
    """``gpcv_step`` for the copula-process ("cv") likelihood, scale(f) = sum_k a_k softplus(b_k f + c_k)
    (include/volt_hip.h, volt_gpcv_cv_step_f32).  abc [B,3,Kc]: the TRANSFORMED a, b, c of every series.
    Returns the workspace: what ``gpcv_step`` returns plus .grad_abc [B,3,Kc] = dF/d(a,b,c)."""
    return _gpcv_dense_step(K, resid, m, Lq, y, abc, gh_x, gh_w, ws, want_dk, jitter, min_var, min_scale, w_ell, w_kl)


def _gpcv_dense_step(K, resid, m, Lq, y, abc, gh_x, gh_w, ws, want_dk, jitter, min_var, min_scale, w_ell, w_kl):
    """`gpcv_step` (``abc`` None: volt_gpcv_step_f32) and `gpcv_cv_step` (volt_gpcv_cv_step_f32, which takes abc, Kc and
    grad_abc besides)."""
    _need_gpu(K, resid, m, Lq, y, abc, gh_x, gh_w)
    if K.ndim != 3 or K.dtype != torch.float32:
        raise ValueError("K must be [B,N,N] fp32")
    B, n, _ = K.shape
    abc, Kc, sizeable = _abc_arg(abc, B, "B")
    if K.stride(-1) != 1:
        K = K.contiguous()
    resid, m, y, Lq = _f32(resid, (B, n)), _f32(m, (B, n)), _f32(y, (B, n)), _f32(Lq, (B, n, n))
    gh_x, gh_w, quad = _quad_args(gh_x, gh_w, min_var, min_scale, w_ell, w_kl)
    ws = _step_workspace(GpcvWorkspace, ws, sizeable, B, n, want_dk, K.device, Kc)
    prior = (K.data_ptr(), K.stride(1), K.stride(0), float(jitter), resid.data_ptr(), m.data_ptr(), Lq.data_ptr(), y.data_ptr())
    grads = _ptrs(ws, "out", "grad_m", "grad_mu", "grad_Lq", "grad_K")
    tail = (*_ptrs(ws, "info", "ptr"), B, n, _lib.WS_INITIALISED if ws is not None else 0, _lib.stream_ptr())
    if abc is None:
        _lib.check(_lib.lib().volt_gpcv_step_f32(*prior, *quad, *grads, *tail), "volt_gpcv_step")
    else:
        _lib.check(_lib.lib().volt_gpcv_cv_step_f32(*prior, abc.data_ptr(), Kc, *quad, *grads, *_ptrs(ws, "grad_abc"), *tail),
                   "volt_gpcv_cv_step")
    return ws


class GpcvBmWorkspace(_GpcvStepWorkspace):
    """Caller-owned scratch and outputs of volt_gpcv_bm_step_f32, reusable across steps of the same (B, N, Kc): one packed
    fp64 triangle per series plus O(B N); no initialisation call.  Kc > 0 adds .grad_abc [B,3,Kc] (the "cv" likelihood)."""

    def __init__(self, B: int, N: int, device, Kc: int = 0):
        self.B, self.N, self.Kc = B, N, self._checked_kc(Kc)
        self._allocate((B, N, self.Kc), device, _lib.lib().volt_gpcv_bm_workspace_bytes(B, N, self.Kc), n_info=B, outputs={
            "out": (B, 12), "grad_m": (B, N), "grad_mu": (B, N), "grad_Lq": (B, N, N), "grad_abc": (B, 3, Kc) if Kc else None})

    def fits(self, B, N, device, Kc=0):
        return self._fits(device, B, N, Kc)


def gpcv_bm_step(x, vol, resid, m, Lq, y, gh_x, gh_w, ws: GpcvBmWorkspace | None = None, abc=None, jitter: float = 1e-3,
                 min_var: float = 1e-6, min_scale: float = 1e-3, w_ell: float = 1.0, w_kl: float = 1.0):
    """``gpcv_step`` / ``gpcv_cv_step`` (abc [B,3,Kc] given) for the Brownian-motion prior K = vol min(x, x') in O(N^2)
    (include/volt_hip.h, volt_gpcv_bm_step_f32): x [N] the grid (0 <= x_0 < x_1 < ..), vol [B] (or one value for all series).
    Returns the workspace: .out [B,12], .grad_m, .grad_mu, .grad_Lq (.grad_abc with abc), .info -- there is no grad_K;
    d/dvol follows from .out[:, 2:9] (variational._dkl_dscale_grad)."""
    _need_gpu(x, vol, resid, m, Lq, y, gh_x, gh_w)
    if Lq.ndim != 3:
        raise ValueError("Lq must be [B,N,N]")
    B, n, _ = Lq.shape
    if x.shape[-1] != n:
        raise ValueError("x and Lq disagree on N")
    x, vol, _ = _bm_args(x, vol, vol, B, torch.float32)
    resid, m, y, Lq = _f32(resid, (B, n)), _f32(m, (B, n)), _f32(y, (B, n)), _f32(Lq, (B, n, n))
    gh_x, gh_w, quad = _quad_args(gh_x, gh_w, min_var, min_scale, w_ell, w_kl)
    abc, Kc, sizeable = _abc_arg(abc, B, "B")
    ws = _step_workspace(GpcvBmWorkspace, ws, sizeable, B, n, Lq.device, Kc)
    with torch.cuda.device(Lq.device):
        _lib.check(_lib.lib().volt_gpcv_bm_step_f32(
            x.data_ptr(), vol.data_ptr(), float(jitter), resid.data_ptr(), m.data_ptr(), Lq.data_ptr(), y.data_ptr(),
            abc.data_ptr() if abc is not None else None, Kc, *quad,
            *_ptrs(ws, "out", "grad_m", "grad_mu", "grad_Lq", "grad_abc", "info", "ptr"), B, n, _lib.stream_ptr()),
            "volt_gpcv_bm_step")
    return ws


class GpcvMarkovWorkspace(_GpcvStepWorkspace):
    """Caller-owned scratch and outputs of volt_gpcv_markov_step_f32, reusable across steps of the same (B, N, Kc): O(B N)
    bytes, no initialisation call.  After a step ``.s`` [B,N] (fp64, a view of the scratch) holds diag S = diag P^-1.
    Kc > 0 adds .grad_abc [B,3,Kc] (the "cv" likelihood)."""

    def __init__(self, B: int, N: int, device, Kc: int = 0):
        self.B, self.N, self.Kc = B, N, self._checked_kc(Kc)
        self._allocate((B, N, self.Kc), device, _lib.lib().volt_gpcv_markov_workspace_bytes(B, N, self.Kc), n_info=B, outputs={
            "out": (B, 12), "grad_m": (B, N), "grad_mu": (B, N), "grad_rho": (B, N), "grad_gamma": (B, N),
            "grad_abc": (B, 3, Kc) if Kc else None})
        off = self.ptr - self.buf.data_ptr()
        self.s = self.buf[off:off + 8 * B * N].view(torch.float64).view(B, N)

    def fits(self, B, N, device, Kc=0):
        return self._fits(device, B, N, Kc)


def gpcv_markov_step(x, vol, resid, m, rho, gamma, y, gh_x, gh_w, ws: GpcvMarkovWorkspace | None = None, abc=None,
                     jitter: float = 1e-3, min_var: float = 1e-6, min_scale: float = 1e-3, w_ell: float = 1.0,
                     w_kl: float = 1.0):
    """The GPCV ELBO step in O(N) for the Markov variational family q = N(m, (Lp Lp')^-1), Lp lower bidiagonal with diagonal
    exp(rho) and sub-diagonal gamma exp(rho), under the Brownian prior started from an N(0, jitter) level,
    K_M = vol min(x, x') + jitter 1 1' -- NOT the other steps' K + jitter I (include/volt_hip.h, volt_gpcv_markov_step_f32).
    x [N] the grid (0 <= x_0 < x_1 < ..), vol [B] (or one value), resid = m - mu, m, rho, gamma, y [B,N] (gamma[:, N-1] is
    not read); abc [B,3,Kc] given: the "cv" likelihood.  Returns the workspace: .out [B,12] (out[:, 6] = dF/dvol,
    out[:, 9] = F), .grad_m, .grad_mu, .grad_rho, .grad_gamma (.grad_abc with abc), .info, .s = diag S."""
    _need_gpu(x, vol, resid, m, rho, gamma, y, gh_x, gh_w, abc)
    if m.ndim != 2:
        raise ValueError("m must be [B,N]")
    B, n = m.shape
    if x.shape[-1] != n:
        raise ValueError("x and m disagree on N")
    x, vol, _ = _bm_args(x, vol, vol, B, torch.float32)
    resid, m, y, rho, gamma = (_f32(t, (B, n)) for t in (resid, m, y, rho, gamma))
    gh_x, gh_w, quad = _quad_args(gh_x, gh_w, min_var, min_scale, w_ell, w_kl)
    abc, Kc, sizeable = _abc_arg(abc, B, "B")
    ws = _step_workspace(GpcvMarkovWorkspace, ws, sizeable, B, n, m.device, Kc)
    with torch.cuda.device(m.device):
        _lib.check(_lib.lib().volt_gpcv_markov_step_f32(
            x.data_ptr(), vol.data_ptr(), float(jitter), resid.data_ptr(), m.data_ptr(), rho.data_ptr(), gamma.data_ptr(),
            y.data_ptr(), abc.data_ptr() if abc is not None else None, Kc, *quad,
            *_ptrs(ws, "out", "grad_m", "grad_mu", "grad_rho", "grad_gamma", "grad_abc", "info", "ptr"), B, n,
            _lib.stream_ptr()), "volt_gpcv_markov_step")
    return ws


class GpcvMarkovNgWorkspace(_GpcvStepWorkspace):
    """Caller-owned scratch and outputs of volt_gpcv_markov_ng_f32, reusable across updates of the same (B, N, Kc): 32 B N
    bytes, no initialisation call.  ``.m_out``, ``.rho_out``, ``.gamma_out`` [B,N] fp32 receive the new q unless the caller
    names other buffers; ``.out`` [B,4] fp64 and ``.info`` [B]; after an update ``.s`` [B,N] (fp64, a view of the scratch)
    holds diag P^-1 of the q that went IN."""
    _STEP = 'the "cv" natural-gradient update'

    def __init__(self, B: int, N: int, device, Kc: int = 0):
        self.B, self.N, self.Kc = B, N, self._checked_kc(Kc)
        self._allocate((B, N, self.Kc), device, _lib.lib().volt_gpcv_markov_ng_workspace_bytes(B, N, self.Kc), n_info=B,
                       outputs={"m_out": (B, N), "rho_out": (B, N), "gamma_out": (B, N)})
        self.out = torch.empty(B, 4, dtype=torch.float64, device=device)
        off = self.ptr - self.buf.data_ptr()
        self.s = self.buf[off:off + 8 * B * N].view(torch.float64).view(B, N)

    def fits(self, B, N, device, Kc=0):
        return self._fits(device, B, N, Kc)


def gpcv_markov_natgrad(x, vol, mu, m, rho, gamma, y, gh_x, gh_w, lam1, lam2, ws: GpcvMarkovNgWorkspace | None = None, abc=None,
                        into=None, jitter: float = 1e-3, min_var: float = 1e-6, min_scale: float = 1e-3, w_ell: float = 1.0,
                        w_kl: float = 1.0, step: float = 1.0):
    """One natural-gradient update of the Markov variational family in O(N) and ONE launch (include/volt_hip.h,
    volt_gpcv_markov_ng_f32).  Arguments as ``gpcv_markov_step`` with the prior mean ``mu`` [B,N] in place of
    resid, and the sites ``lam1``, ``lam2`` [B,N] fp64 contiguous, UPDATED IN PLACE (zeros: q = prior): they move ``step`` in
    (0, 1] towards t2 = max(-2 r dE/ds, 0), t1 = r dE/dm + t2 (m - mu), r = w_ell / w_kl, and the q with precision
    K_M^-1 + diag(lam2) and mean mu + P^-1 lam1 is written to ``into`` = (m_out, rho_out, gamma_out), fp32 contiguous [B,N]
    -- they MAY be m, rho, gamma themselves -- or, without ``into``, to the workspace's .m_out, .rho_out, .gamma_out.
    Returns the workspace: .out [B,4] fp64 = (clamped sites, max |dm|, max |drho|, max |dgamma|), .info (1: a non-finite
    series, whose outputs and sites are NaN), .s = diag P^-1 of the q that went in.  No host read."""
    _need_gpu(x, vol, mu, m, rho, gamma, y, gh_x, gh_w, lam1, lam2, abc)
    if m.ndim != 2:
        raise ValueError("m must be [B,N]")
    B, n = m.shape
    if x.shape[-1] != n:
        raise ValueError("x and m disagree on N")
    for name, t in (("lam1", lam1), ("lam2", lam2)):
        if t.dtype != torch.float64 or tuple(t.shape) != (B, n) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp64 [B,N] = {(B, n)} tensor (it is updated in place)")
    if not 0.0 < float(step) <= 1.0:
        raise ValueError(f"gpcv_markov_natgrad: step must lie in (0, 1], got {step}")
    x, vol, _ = _bm_args(x, vol, vol, B, torch.float32)
    mu = mu.detach().to(torch.float32)                                   # [B,N], or one value per series, or one value
    mu = (mu.reshape(B, n) if mu.numel() == B * n else mu.reshape(-1, 1).expand(B, n)).contiguous()
    m, y, rho, gamma = (_f32(t, (B, n)) for t in (m, y, rho, gamma))
    gh_x, gh_w, quad = _quad_args(gh_x, gh_w, min_var, min_scale, w_ell, w_kl)
    abc, Kc, sizeable = _abc_arg(abc, B, "B", reject=GpcvMarkovNgWorkspace._STEP)
    ws = _step_workspace(GpcvMarkovNgWorkspace, ws, sizeable, B, n, m.device, Kc)
    if into is None:
        into = (ws.m_out, ws.rho_out, ws.gamma_out)
    for t in into:
        if t.dtype != torch.float32 or tuple(t.shape) != (B, n) or not t.is_contiguous() or t.device != m.device:
            raise ValueError(f"gpcv_markov_natgrad: every output must be a contiguous fp32 [B,N] = {(B, n)} tensor on m's device")
    with torch.cuda.device(m.device):
        _lib.check(_lib.lib().volt_gpcv_markov_ng_f32(
            x.data_ptr(), vol.data_ptr(), float(jitter), mu.data_ptr(), m.data_ptr(), rho.data_ptr(), gamma.data_ptr(),
            y.data_ptr(), abc.data_ptr() if abc is not None else None, Kc, *quad, float(step), lam1.data_ptr(), lam2.data_ptr(),
            *(t.data_ptr() for t in into), *_ptrs(ws, "out", "info", "ptr"), B, n, _lib.stream_ptr()),
            "volt_gpcv_markov_natgrad")
    return ws


def _markov_root_args(rho, gamma):
    _need_gpu(rho, gamma)
    if rho.ndim != 2 or gamma.shape != rho.shape:
        raise ValueError("rho and gamma must both be [B,N]")
    return rho.to(torch.float32).contiguous(), gamma.to(torch.float32).contiguous()


def markov_root_draw(m: torch.Tensor, rho: torch.Tensor, gamma: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
    """m + Lp^-T eps for the bidiagonal precision root Lp of (rho, gamma) (volt_markov_root_draw_f32): m, rho, gamma [B,N],
    eps [B,reps,N] -> [B,reps,N]; one backward affine recurrence per draw, fp64 arithmetic rounded once."""
    rho, gamma = _markov_root_args(rho, gamma)
    _need_gpu(m, eps)
    B, n = rho.shape
    if eps.ndim != 3 or eps.shape[0] != B or eps.shape[2] != n or eps.shape[1] < 1 or tuple(m.shape) != (B, n):
        raise ValueError(f"m must be [B,N] = {(B, n)} and eps [B,reps,N]")
    m, eps = m.to(torch.float32).contiguous(), eps.to(torch.float32).contiguous()
    out = torch.empty_like(eps)
    with torch.cuda.device(eps.device):
        _lib.check(_lib.lib().volt_markov_root_draw_f32(m.data_ptr(), rho.data_ptr(), gamma.data_ptr(), eps.data_ptr(),
                                                        out.data_ptr(), B, eps.shape[1], n, _lib.stream_ptr()),
                   "volt_markov_root_draw")
    return out


def markov_root_var(rho: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    """diag (Lp Lp')^-1 [B,N] in fp64 (volt_markov_root_var_f32): the s of ``gpcv_markov_step``."""
    rho, gamma = _markov_root_args(rho, gamma)
    B, n = rho.shape
    var = torch.empty(B, n, dtype=torch.float64, device=rho.device)
    with torch.cuda.device(rho.device):
        _lib.check(_lib.lib().volt_markov_root_var_f32(rho.data_ptr(), gamma.data_ptr(), var.data_ptr(), B, n,
                                                       _lib.stream_ptr()), "volt_markov_root_var")
    return var


class MarkovPredictPlan:
    """What ``markov_predict_plan`` returns.  In the CALLER's order of the test points: ``mean``, ``var_q`` (the q part
    A P^-1 A'), ``var_p`` (the bridge part K** - A K_uu A') [B,H] fp64.  ``info`` [B] int32 (0; -(h + 1): the h-th point of the
    SORTED list is NaN, infinite, negative -- the series' results are then NaN; 1: a variance is not finite).  The draw plan
    itself (``coef``, ``code``, ``steps``, over the sorted points) is for ``markov_predict_draw``; ``E``: the base samples a
    path consumes, <= 3 H + 1 -- read from the device once (ONE HOST SYNCHRONISATION, at the first use: code that sizes its base
    samples by it cannot be captured in a graph unless E was read before the capture; ``steps`` depends on (x, xs) alone)."""

    def __init__(self, B, N, H, mean, var_q, var_p, coef, code, steps, info, order):
        self.B, self.N, self.H = B, N, H
        self._mean, self._var_q, self._var_p = mean, var_q, var_p      # (over the sorted points)
        self.coef, self.code, self.steps, self.info, self.order = coef, code, steps, info, order
        self._E = None

    def _caller_order(self, t):
        out = torch.empty_like(t)
        out[:, self.order] = t
        return out

    mean = property(lambda self: self._caller_order(self._mean))
    var_q = property(lambda self: self._caller_order(self._var_q))
    var_p = property(lambda self: self._caller_order(self._var_p))

    @property
    def E(self):
        if self._E is None:
            self._E = int(self.steps.max().item())
        return self._E


def markov_predict_plan(x, xs, vol, mu, m, rho, gamma, jitter: float = 1e-3) -> MarkovPredictPlan:
    """The Markov GPCV's q(f(xs)) at H test points away from its grid, in O(N + H log N) per series and ONE launch
    (volt_markov_predict_plan_f32): x [N] the grid, xs [H] the test points in ANY order (sorted here, stably; every
    result comes back in the caller's order), >= 0; vol, mu [B] (or one value): the prior's scale and constant; m, rho, gamma
    [B,N] the family's parameters (gamma[:, N-1] is not read); jitter: the prior's level variance.  No gradients."""
    _need_gpu(x, xs, vol, mu, m, rho, gamma)
    if m.ndim != 2 or rho.shape != m.shape or gamma.shape != m.shape:
        raise ValueError("m, rho and gamma must all be [B,N]")
    B, n = m.shape
    if x.ndim != 1 or x.shape[0] != n:
        raise ValueError("x must be [N] with m's N")
    if xs.ndim != 1 or xs.shape[0] < 1:
        raise ValueError("xs must be [H], H >= 1")
    H = xs.shape[0]
    nbytes = _lib.lib().volt_markov_predict_workspace_bytes(B, n, H)
    if nbytes == 0:
        raise ValueError(f"markov_predict_plan: (B, N, H) = {(B, n, H)} is out of range (1 <= B <= 65535, N >= 1, 1 <= H <= 2^24)")
    dev = m.device
    xs_sorted, order = torch.sort(xs.detach().to(torch.float32), stable=True)
    x = x.detach().to(torch.float32).contiguous()
    vol, mu = (torch.as_tensor(t, device=dev).detach().to(torch.float32).reshape(-1).expand(B).contiguous() for t in (vol, mu))
    m, rho, gamma = (_f32(t, (B, n)) for t in (m, rho, gamma))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    mean, var_q, var_p, coef = f64(B, H), f64(B, H), f64(B, H), f64(B, 3 * H + 1, 3)
    code, steps, info = i32(B, 3 * H + 1), i32(B), i32(B)
    _, ws = _scratch(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().volt_markov_predict_plan_f32(
            x.data_ptr(), xs_sorted.data_ptr(), vol.data_ptr(), float(jitter), mu.data_ptr(), m.data_ptr(), rho.data_ptr(),
            gamma.data_ptr(), mean.data_ptr(), var_q.data_ptr(), var_p.data_ptr(), coef.data_ptr(), code.data_ptr(),
            steps.data_ptr(), info.data_ptr(), ws, B, n, H, _lib.stream_ptr()), "volt_markov_predict_plan")
    return MarkovPredictPlan(B, n, H, mean, var_q, var_p, coef, code, steps, info, order)


_PREDICT_PARTS = {"both": 0, "chain": _lib.PREDICT_NO_BRIDGE, "bridge": _lib.PREDICT_NO_CHAIN}


def markov_predict_draw(plan: MarkovPredictPlan, eps: torch.Tensor, exp: bool = False, part: str = "both") -> torch.Tensor:
    """Joint draws of f at the plan's test points in O(S H) (volt_markov_predict_draw_f32): eps [B,S,E'] with E' >= plan.E base
    samples per path (N(0,1) for a draw; columns beyond plan.E are not read) -> [B,S,H] fp32 in the caller's order of the test
    points.  ``exp``: the exponential of the draw, computed in double and rounded once.  ``part``: "both"; "chain": mean + the
    q part alone (covariance A P^-1 A'); "bridge": mean + the bridge part alone (K** - A K_uu A') -- the two use disjoint
    columns of eps.  A series whose plan failed (plan.info < 0) comes back NaN."""
    _need_gpu(eps)
    if part not in _PREDICT_PARTS:
        raise ValueError(f"part must be one of {tuple(_PREDICT_PARTS)}, got {part!r}")
    if eps.ndim != 3 or eps.shape[0] != plan.B or eps.shape[1] < 1 or eps.shape[2] < 1:
        raise ValueError(f"eps must be [B,S,E] with B = {plan.B}")
    _, S, E = eps.shape
    eps = eps.detach().to(torch.float32).contiguous()
    out = torch.empty(plan.B, S, plan.H, dtype=torch.float32, device=eps.device)
    with torch.cuda.device(eps.device):
        _lib.check(_lib.lib().volt_markov_predict_draw_f32(
            plan._mean.data_ptr(), plan.coef.data_ptr(), plan.code.data_ptr(), plan.steps.data_ptr(), eps.data_ptr(),
            out.data_ptr(), plan.B, S, plan.H, E, (_lib.DRAW_EXP if exp else 0) | _PREDICT_PARTS[part], _lib.stream_ptr()),
            "volt_markov_predict_draw")
    if plan.H > 1:                                                     # back to the caller's order
        res = torch.empty_like(out)
        res[:, :, plan.order] = out
        return res
    return out


GPCV_MT_T_MAX = 64                 # include/volt_hip.h: volt_gpcv_mt_step_f32 takes 1 <= T <= 64 series


class GpcvMtWorkspace(_GpcvStepWorkspace):
    """Caller-owned scratch and outputs of volt_gpcv_mt_step_f32, reusable across steps of the same (N, T).
    Kc > 0: the workspace of volt_gpcv_mt_cv_step_f32 for Kc warp terms per task (adds .grad_abc [T,3,Kc]).
    info[0]: the factorisation of K + jitter I; info[1]: a non-positive pivot of K_t; info[2]: F is not finite."""
    _STEP = 'the "cv" multi-task GPCV step'

    def __init__(self, N: int, T: int, want_dk: bool, device, Kc: int = 0):
        if T < 1 or T > GPCV_MT_T_MAX:
            raise ValueError(f"the multi-task GPCV step takes 1 <= T <= {GPCV_MT_T_MAX} series (got T = {T})")
        self.N, self.T, self.want_dk, self.Kc = N, T, bool(want_dk), self._checked_kc(Kc)
        L = _lib.lib()
        nbytes = L.volt_gpcv_mt_cv_workspace_bytes(N, T, int(want_dk), self.Kc) if Kc else L.volt_gpcv_mt_workspace_bytes(N, T, int(want_dk))
        # (the MLL workspace it begins with is for ONE series)
        self._allocate((N, T, self.want_dk, self.Kc), device, nbytes, mll_init=(1, N), n_info=3, outputs={
            "out": (16,), "grad_M": (N, T), "grad_c": (T,), "grad_Lx": (N, N), "grad_Lt": (T, T), "grad_covar_factor": (T,),
            "grad_raw_var": (T,), "grad_K": (N, N) if want_dk else None, "grad_abc": (T, 3, Kc) if Kc else None})

    def fits(self, N, T, want_dk, device, Kc=0):
        return self._fits(device, N, T, bool(want_dk), Kc)


def gpcv_mt_step(K, M, c, Lx, Lt, covar_factor, raw_var, y, gh_x, gh_w, ws: GpcvMtWorkspace | None = None,
                 want_dk: bool = False, jitter: float = 1e-3, min_var: float = 1e-6, min_scale: float = 1e-3,
                 w_ell: float = 1.0, w_kl: float = 1.0, abc=None):
    """One ELBO + gradient evaluation of the multi-task GPCV variational GP (include/volt_hip.h, volt_gpcv_mt_step_f32).
    K [N,N] data prior covariance without jitter; M, y [N,T]; c, covar_factor ([T] or [T,1]), raw_var [T]; Lx [N,N],
    Lt [T,T] (what lies above their diagonals is ignored).  Gradients are those of F = w_ell * ell - w_kl * KL (out[12]).
    abc None: the "exp" likelihood.  abc [T,3,Kc]: the copula-process ("cv") likelihood with the TRANSFORMED a, b, c of
    every task, scale_t(f) = sum_k a_tk softplus(b_tk f + c_tk) (volt_gpcv_mt_cv_step_f32).
    Returns the workspace: .out [16], .grad_M, .grad_c, .grad_Lx, .grad_Lt, .grad_covar_factor, .grad_raw_var
    (.grad_K if want_dk, .grad_abc [T,3,Kc] = dF/d(a,b,c) with abc), .info [3]."""
    _need_gpu(K, M, c, Lx, Lt, covar_factor, raw_var, y, abc, gh_x, gh_w)
    if K.ndim != 2 or K.dtype != torch.float32:
        raise ValueError("K must be [N,N] fp32")
    n = K.shape[0]
    T = M.shape[-1]
    if K.stride(-1) != 1:
        K = K.contiguous()
    M, y, Lx, Lt = _f32(M, (n, T)), _f32(y, (n, T)), _f32(Lx, (n, n)), _f32(Lt, (T, T))
    c, cf, rv = _f32(c, (T,)), _f32(covar_factor, (T,)), _f32(raw_var, (T,))
    gh_x, gh_w, quad = _quad_args(gh_x, gh_w, min_var, min_scale, w_ell, w_kl)
    abc, Kc, sizeable = _abc_arg(abc, T, "T", reject=GpcvMtWorkspace._STEP)
    ws = _step_workspace(GpcvMtWorkspace, ws, sizeable, n, T, want_dk, K.device, Kc)
    prior = (K.data_ptr(), K.stride(0), float(jitter), M.data_ptr(), c.data_ptr(), Lx.data_ptr(), Lt.data_ptr(), cf.data_ptr(),
             rv.data_ptr(), y.data_ptr())
    grads = _ptrs(ws, "out", "grad_M", "grad_c", "grad_Lx", "grad_Lt", "grad_covar_factor", "grad_raw_var", "grad_K")
    tail = (*_ptrs(ws, "info", "ptr"), n, T, _lib.WS_INITIALISED, _lib.stream_ptr())
    if abc is None:
        _lib.check(_lib.lib().volt_gpcv_mt_step_f32(*prior, *quad, *grads, *tail), "volt_gpcv_mt_step")
    else:
        _lib.check(_lib.lib().volt_gpcv_mt_cv_step_f32(*prior, abc.data_ptr(), Kc, *quad, *grads, *_ptrs(ws, "grad_abc"), *tail),
                   "volt_gpcv_mt_cv_step")
    return ws


class GpcvMtMarkovWorkspace(_GpcvStepWorkspace):
    """Caller-owned scratch and outputs of volt_gpcv_mt_markov_step_f32, reusable across steps of the same (N, T, Kc):
    O(N T + T^2 N / 128) bytes, no initialisation call.  After a step ``.s`` [N] (fp64, a view of the scratch) holds
    diag P^-1.  Kc > 0 adds .grad_abc [T,3,Kc] (the "cv" likelihood, one warp per task).
    info[0]: F is not finite; info[1]: a non-positive pivot of K_t."""
    _STEP = 'the "cv" multi-task GPCV step (markov family)'

    def __init__(self, N: int, T: int, device, Kc: int = 0):
        if T < 1 or T > GPCV_MT_T_MAX:
            raise ValueError(f"the multi-task GPCV step takes 1 <= T <= {GPCV_MT_T_MAX} series (got T = {T})")
        self.N, self.T, self.Kc = N, T, self._checked_kc(Kc)
        self._allocate((N, T, self.Kc), device, _lib.lib().volt_gpcv_mt_markov_workspace_bytes(N, T, self.Kc), n_info=2, outputs={
            "out": (12,), "grad_M": (N, T), "grad_c": (T,), "grad_rho": (N,), "grad_gamma": (N,), "grad_Lt": (T, T),
            "grad_covar_factor": (T,), "grad_raw_var": (T,), "grad_abc": (T, 3, Kc) if Kc else None})
        off = self.ptr - self.buf.data_ptr()
        self.s = self.buf[off:off + 8 * N].view(torch.float64)

    def fits(self, N, T, device, Kc=0):
        return self._fits(device, N, T, Kc)


def gpcv_mt_markov_step(x, vol, M, c, rho, gamma, Lt, covar_factor, raw_var, y, gh_x, gh_w,
                        ws: GpcvMtMarkovWorkspace | None = None, abc=None, jitter: float = 1e-3, min_var: float = 1e-6,
                        min_scale: float = 1e-3, w_ell: float = 1.0, w_kl: float = 1.0):
    """The multi-task GPCV ELBO step in O(N T) for the Markov family q(F) = N(M, (Lp Lp')^-1 (x) Lt Lt') under the prior
    N(1 c', K_M (x) K_t), K_M = vol min(x, x') + jitter 1 1' (include/volt_hip.h, volt_gpcv_mt_markov_step_f32).
    x [N] the grid (0 <= x_0 < x_1 < ..), vol one value, M, y [N,T], c, covar_factor ([T] or [T,1]), raw_var [T], rho, gamma [N]
    (gamma[N-1] is not read), Lt [T,T] (what lies above its diagonal is ignored); abc [T,3,Kc] given: the "cv" likelihood
    with the TRANSFORMED a, b, c of every task.  Gradients are those of F = w_ell * ell - w_kl * KL (out[10]).
    Returns the workspace: .out [12] (out[9] = dF/dvol), .grad_M, .grad_c, .grad_rho, .grad_gamma, .grad_Lt,
    .grad_covar_factor, .grad_raw_var (.grad_abc with abc), .info [2], .s = diag P^-1."""
    _need_gpu(x, vol, M, c, rho, gamma, Lt, covar_factor, raw_var, y, abc, gh_x, gh_w)
    if M.ndim != 2:
        raise ValueError("M must be [N,T]")
    n, T = M.shape
    if x.shape[-1] != n or x.numel() != n:
        raise ValueError("x and M disagree on N")
    x, vol, _ = _bm_args(x, vol, vol, 1, torch.float32)
    M, y, Lt = _f32(M, (n, T)), _f32(y, (n, T)), _f32(Lt, (T, T))
    rho, gamma = _f32(rho, (n,)), _f32(gamma, (n,))
    c, cf, rv = _f32(c, (T,)), _f32(covar_factor, (T,)), _f32(raw_var, (T,))
    gh_x, gh_w, quad = _quad_args(gh_x, gh_w, min_var, min_scale, w_ell, w_kl)
    abc, Kc, sizeable = _abc_arg(abc, T, "T", reject=GpcvMtMarkovWorkspace._STEP)
    ws = _step_workspace(GpcvMtMarkovWorkspace, ws, sizeable, n, T, M.device, Kc)
    with torch.cuda.device(M.device):
        _lib.check(_lib.lib().volt_gpcv_mt_markov_step_f32(
            x.data_ptr(), vol.data_ptr(), float(jitter), M.data_ptr(), c.data_ptr(), rho.data_ptr(), gamma.data_ptr(),
            Lt.data_ptr(), cf.data_ptr(), rv.data_ptr(), y.data_ptr(), abc.data_ptr() if abc is not None else None, Kc, *quad,
            *_ptrs(ws, "out", "grad_M", "grad_c", "grad_rho", "grad_gamma", "grad_Lt", "grad_covar_factor", "grad_raw_var",
                   "grad_abc", "info", "ptr"), n, T, _lib.stream_ptr()), "volt_gpcv_mt_markov_step")
    return ws


def mll_grad_k(ws: MllWorkspace) -> torch.Tensor:
    """d mll / d K = 1/2 (alpha alpha' - K_s^-1) / N  [B,N,N], from the Y = L^-T the last ``mll_step(want_grad=True)``
    left in ``ws`` (volt_mll_grad_k_f32) -- for kernels with trainable parameters."""
    if not ws.want_grad:
        raise ValueError("mll_grad_k needs a workspace used with want_grad=True")
    B, n = ws.B, ws.N
    Np = padded_n(n)
    scratch = torch.empty(B, Np, Np, dtype=torch.float32, device=ws.buf.device)
    gK = torch.empty(B, n, n, dtype=torch.float32, device=ws.buf.device)
    _lib.check(_lib.lib().volt_mll_grad_k_f32(ws.ptr, ws.alpha.data_ptr(), scratch.data_ptr(), gK.data_ptr(), B, n,
                                              _lib.stream_ptr()), "volt_mll_grad_k")
    return gK


# ------------------------------------------------------------------ Kronecker multi-task vol forecaster (MultitaskBMGP)
KRON_T_MAX = 64                     # include/volt_hip.h: volt_syev_small_f64 / volt_kron_*: T <= 64
# The T steps of one Kronecker iteration all factor M + sigma_j^2 I over the SAME M: it is handed to the step with batch
# stride 0 (no [T,N,N] copy) -- the step only reads K, and tests/test_gpu_multitask.py checks that this gives bitwise the
# result of T materialised copies.
KRON_SHARED_K = True


def _check_tasks(T: int):
    if T < 1 or T > KRON_T_MAX:
        raise ValueError(f"the Kronecker multi-task path takes 1 <= T <= {KRON_T_MAX} tasks (got T = {T})")


def syev_small(S: torch.Tensor):
    """Eigendecomposition of symmetric [B,T,T] (or [T,T]) fp64 matrices, T <= 64 (volt_syev_small_f64: parallel cyclic
    Jacobi, one workgroup per matrix).  Returns (lam [B,T] ascending, Q [B,T,T] with the eigenvectors as columns, info [B]
    = sweeps used, -1 if the sweep cap was hit)."""
    _need_gpu(S)
    two_d = S.ndim == 2
    S3 = (S.unsqueeze(0) if two_d else S).to(torch.float64).contiguous()
    B, T = S3.shape[0], S3.shape[-1]
    _check_tasks(T)
    lam = torch.empty(B, T, dtype=torch.float64, device=S.device)
    Q = torch.empty(B, T, T, dtype=torch.float64, device=S.device)
    info = torch.empty(B, dtype=torch.int32, device=S.device)
    _lib.check(_lib.lib().volt_syev_small_f64(S3.data_ptr(), T * T, lam.data_ptr(), Q.data_ptr(), info.data_ptr(), B, T,
                                              _lib.stream_ptr()), "volt_syev_small_f64")
    return (lam[0], Q[0], info[0]) if two_d else (lam, Q, info)


KRON_SOLVERS = ("dense", "linear")
KRON_EPILOGUE_SLICE = 256           # include/volt_hip.h: columns of N per workgroup of volt_kron_epilogue_ws_*'s first launch


class KronWorkspace:
    """Caller-owned buffers of one Kronecker MLL iteration of shape (N, T, dtype): the prologue's state (fp64: vol, Lambda,
    d, W, Q), the step's inputs (resid [T,N], sigma2 [T]) and workspace (B = T, with gradient), the eigensolver's info
    and the epilogue's packed result res [3 + 3T].  ``solver="linear"`` (`kron_bm_step`): the step's workspace is a
    BmWorkspace(T, N) instead of the MllWorkspace, beside it the step's ``ones`` [T] (its vol) and the scratch of the split
    epilogue -- O(T N + T^2 N / 256) in all, never an N x N buffer."""

    def __init__(self, N: int, T: int, device, dtype=torch.float32, solver: str = "dense"):
        _check_tasks(T)
        if solver not in KRON_SOLVERS:
            raise ValueError(f"KronWorkspace: solver must be one of {KRON_SOLVERS}, got {solver!r}")
        self.N, self.T, self.dtype, self.solver = N, T, dtype, solver
        L = _lib.lib()
        self.state = torch.zeros(int(L.volt_kron_state_bytes(T)) // 8, dtype=torch.float64, device=device)
        self.resid = torch.empty(T, N, dtype=dtype, device=device)
        self.sigma2 = torch.empty(T, dtype=dtype, device=device)
        self.eig_info = torch.zeros(1, dtype=torch.int32, device=device)
        self.res = torch.empty(3 + 3 * T, dtype=dtype, device=device)
        if solver == "linear":
            self.bm = BmWorkspace(T, N, device, dtype)
            self.ones = torch.ones(T, dtype=dtype, device=device)
            self.epi_buf, self.epi_ptr = _scratch(int(L.volt_kron_epilogue_workspace_bytes(N, T)), device)
        else:
            self.mll = MllWorkspace(T, N, True, device, dtype)
        self._K = None

    def fits(self, N, T, device, dtype=torch.float32, solver="dense"):
        return (self.N, self.T, self.state.device, self.dtype, self.solver) == (N, T, device, dtype, solver)

    def shared_k(self, M: torch.Tensor) -> torch.Tensor:
        """M as the step's [T,N,N] operand: batch stride 0 (KRON_SHARED_K), or T copies made once per M."""
        if KRON_SHARED_K:
            return M.expand(self.T, self.N, self.N)
        if self._K is None or self._K[0] is not M:
            self._K = (M, M.expand(self.T, self.N, self.N).contiguous())
        return self._K[1]

    # views of the state (include/volt_hip.h: vol, Lambda [T], d [T], W [T,T], Q [T,T])
    def lam(self):
        return self.state[8: 8 + self.T]

    def d(self):
        return self.state[8 + self.T: 8 + 2 * self.T]

    def W(self):
        T = self.T
        return self.state[8 + 2 * T: 8 + 2 * T + T * T].view(T, T)

    def Q(self):
        T = self.T
        return self.state[8 + 2 * T + T * T: 8 + 2 * T + 2 * T * T].view(T, T)


def _kron_params(params, dt):
    out = []
    for p in params:
        p = p.detach().reshape(-1)
        out.append(p if p.dtype == dt and p.is_contiguous() else p.to(dt).contiguous())
    return out


def kron_prologue(params, x: torch.Tensor, Y: torch.Tensor, ws: KronWorkspace, warm: bool = False):
    """volt_kron_prologue_*: params = (raw_vol [1], covar_factor [T,1], raw_var [T], raw_task_noises [T], raw_noise [1]),
    x [N], Y [N,T] -> ws.resid, ws.sigma2, ws.state, ws.eig_info.  ``warm``: volt_kron_prologue_warm_* -- the same outputs in
    two launches, the eigensolver started from the Q the previous call left in ws.state (cold on a fresh workspace)."""
    _need_gpu(x, Y, *params)
    dt = ws.dtype
    rv, cf, var, rtn, rn = _kron_params(params, dt)
    x = x.reshape(-1).to(dt).contiguous()
    Y = Y.to(dt)
    if Y.stride(-1) != 1:
        Y = Y.contiguous()
    N, T = ws.N, ws.T
    if tuple(Y.shape) != (N, T) or x.numel() != N or cf.numel() != T:
        raise ValueError(f"kron_prologue: x [N], Y [N,T] and covar_factor [T,1] must agree with the workspace (N={N}, T={T})")
    fn = getattr(_lib.lib(), ("volt_kron_prologue_warm" if warm else "volt_kron_prologue") + ("_f32" if dt == torch.float32 else "_f64"))
    _lib.check(fn(rv.data_ptr(), cf.data_ptr(), var.data_ptr(), rtn.data_ptr(), rn.data_ptr(), x.data_ptr(), Y.data_ptr(),
                  Y.stride(0), ws.resid.data_ptr(), ws.sigma2.data_ptr(), ws.state.data_ptr(), ws.eig_info.data_ptr(), N, T,
                  _lib.stream_ptr()), "volt_kron_prologue")
    return ws


def kron_mll_step(params, x: torch.Tensor, Y: torch.Tensor, M: torch.Tensor, ws: KronWorkspace | None = None):
    """One Kronecker MLL + gradient evaluation: prologue -> the existing batched step (B = T, K = M, sigma2 = 1 / kappa)
    -> epilogue.  params as for `kron_prologue`; M [N,N] = min(x_i, x_k) in the step's dtype (fp32 or fp64).  Returns
    (res [3 + 3T], step info [T], eigensolver info [1], ws); res = mll, d/d raw_vol, d/d raw_noise, d/d covar_factor [T],
    d/d raw_var [T], d/d raw_task_noises [T] (include/volt_hip.h)."""
    _need_gpu(x, Y, M, *params)
    dt = torch.float64 if M.dtype == torch.float64 else torch.float32
    N, T = Y.shape
    _check_tasks(T)
    if ws is None or not ws.fits(N, T, M.device, dt):
        ws = KronWorkspace(N, T, M.device, dt)
    M = M.to(dt)
    if M.stride(-1) != 1:
        M = M.contiguous()
    kron_prologue(params, x, Y, ws)
    out, alpha, info = mll_step(ws.shared_k(M), ws.resid, ws.sigma2, ws.mll, want_grad=True)
    rv, cf, var, rtn, rn = _kron_params(params, dt)
    xd = x.reshape(-1).to(dt).contiguous()
    fn = _lib.lib().volt_kron_epilogue_f32 if dt == torch.float32 else _lib.lib().volt_kron_epilogue_f64
    _lib.check(fn(rv.data_ptr(), cf.data_ptr(), var.data_ptr(), rtn.data_ptr(), rn.data_ptr(), xd.data_ptr(),
                  ws.resid.data_ptr(), out.data_ptr(), alpha.data_ptr(), ws.state.data_ptr(), ws.res.data_ptr(), N, T,
                  _lib.stream_ptr()), "volt_kron_epilogue")
    return ws.res, info, ws.eig_info, ws


def kron_bm_step(params, x: torch.Tensor, Y: torch.Tensor, ws: KronWorkspace | None = None):
    """`kron_mll_step` without M, in O(T N + T^2 N): warm prologue -> the linear-time chain step (`bm_step` over the grid x
    with vol = 1, sigma2 = 1 / kappa, B = T) -> the epilogue with its N-reductions spread over workgroups
    (volt_kron_epilogue_ws_*).  x [N] must be a valid chain grid (x_0 >= 0, strictly increasing: gp.check_grid); the dtype is
    Y's (fp32 or fp64).  Returns what `kron_mll_step` returns; ``ws`` is a KronWorkspace(solver="linear") and carries the
    eigenvectors from one call to the next."""
    _need_gpu(x, Y, *params)
    dt = torch.float64 if Y.dtype == torch.float64 else torch.float32
    N, T = Y.shape
    _check_tasks(T)
    if ws is None or not ws.fits(N, T, Y.device, dt, "linear"):
        ws = KronWorkspace(N, T, Y.device, dt, "linear")
    xd = x.reshape(-1).to(dt).contiguous()
    with torch.cuda.device(Y.device):
        kron_prologue(params, xd, Y, ws, warm=True)
        out, alpha, info = bm_step(xd, ws.ones, ws.sigma2, ws.resid, ws.bm, want_grad=True)
        rv, cf, var, rtn, rn = _kron_params(params, dt)
        fn = _lib.lib().volt_kron_epilogue_ws_f32 if dt == torch.float32 else _lib.lib().volt_kron_epilogue_ws_f64
        _lib.check(fn(rv.data_ptr(), cf.data_ptr(), var.data_ptr(), rtn.data_ptr(), rn.data_ptr(), xd.data_ptr(),
                      ws.resid.data_ptr(), out.data_ptr(), alpha.data_ptr(), ws.state.data_ptr(), ws.res.data_ptr(), ws.epi_ptr,
                      N, T, _lib.stream_ptr()), "volt_kron_epilogue_ws")
    return ws.res, info, ws.eig_info, ws


# ---- path summaries (volt_path_summary_f32) ---------------------------------------------------------------------------
SUMMARY_MAX_S = _lib.SUMMARY_MAX_S
_SUMMARY_SCRATCH = {}
_SUMMARY_LEVELS = {}


def _summary_scratch(G: int, S: int, H: int, device):
    """Caller-owned scratch of volt_path_summary_f32 (the transposed samples), one buffer per (device, stream, shape),
    reused across calls; calls that share a buffer are ordered by their stream.  Returns (aligned pointer, bytes)."""
    nbytes = int(_lib.lib().volt_path_summary_scratch_bytes(G, S, H))
    return _cached_scratch(_SUMMARY_SCRATCH, (device.index, _lib.stream_ptr(), G, S, H), nbytes, device)[0], nbytes


def _summary_levels(q, device) -> torch.Tensor:
    """The quantile levels as a device fp64 tensor, cached per (levels, device): a host-to-device copy per call would
    keep the entry out of a captured iteration."""
    if torch.is_tensor(q):
        return q.to(device=device, dtype=torch.float64).reshape(-1).contiguous()
    key = (tuple(float(v) for v in q), str(device))
    if key not in _SUMMARY_LEVELS:
        if any(not 0.0 <= v <= 1.0 for v in key[0]):
            raise ValueError("quantile levels must lie in [0, 1]")
        _SUMMARY_LEVELS[key] = torch.tensor(key[0], dtype=torch.float64, device=device)
    return _SUMMARY_LEVELS[key]


def path_summary(samples: torch.Tensor, q=(), truth: torch.Tensor | None = None, strikes: torch.Tensor | None = None,
                 exp: bool = False):
    """volt_path_summary_f32 on samples [G,S,H] (fp32; any view with a contiguous last dimension, a row stride >= H and a
    batch stride is read in place, anything else is copied first).  q: levels (sequence or tensor); truth [G,H] in value
    units; strikes [G,M].  Returns (moments [G,4,H], quant [G,Q,H], counts [G,3,H] int32, crps [G,H], call [G,M,H],
    put [G,M,H]) on the device; no host synchronisation."""
    if samples.ndim != 3:
        raise ValueError("samples must be [G,S,H]")
    G, S, H = samples.shape
    if S > SUMMARY_MAX_S:
        raise ValueError(f"path_summary sorts a column in one workgroup: S = {S} > {SUMMARY_MAX_S}")
    if min(G, S, H) < 1:
        raise ValueError("samples must not be empty")
    _need_gpu(samples, truth, strikes)
    if samples.dtype != torch.float32:
        samples = samples.float()
    sg, ss, sh = samples.stride()
    if (H > 1 and sh != 1) or (S > 1 and ss < H) or (G > 1 and sg < 0):
        samples = samples.contiguous()
        sg, ss, sh = samples.stride()
    ld = ss if S > 1 else H
    dev = samples.device
    f32 = dict(dtype=torch.float32, device=dev)
    qd = _summary_levels(q, dev)
    Q = qd.numel()
    M = 0
    if strikes is not None:
        strikes = strikes.to(torch.float32).reshape(G, -1).contiguous()
        M = strikes.shape[1]
    if truth is not None:
        truth = truth.to(torch.float32).reshape(G, H).contiguous()
    moments = torch.empty(G, 4, H, **f32)
    quant = torch.empty(G, Q, H, **f32)
    counts = torch.empty(G, 3, H, dtype=torch.int32, device=dev)
    crps = torch.empty(G, H, **f32)
    call = torch.empty(G, M, H, **f32)
    put = torch.empty(G, M, H, **f32)
    wp, nbytes = _summary_scratch(G, S, H, dev)

    def P(t, n=1):
        return None if t is None or n == 0 else t.data_ptr()
    _lib.check(_lib.lib().volt_path_summary_f32(
        samples.data_ptr(), ld, sg if G > 1 else 0, G, S, H, _lib.SUMMARY_EXP if exp else 0, P(qd, Q), Q, P(truth),
        P(strikes, M), M, moments.data_ptr(), P(quant, Q), counts.data_ptr(), crps.data_ptr(), P(call, M), P(put, M), wp,
        nbytes, _lib.stream_ptr()), "volt_path_summary")
    return moments, quant, counts, crps, call, put
