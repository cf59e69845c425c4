"""volt_rollout_bordered_f32 and volt_rollout_shared_f32 (csrc/rollout.hip) called directly through _lib, as
rollout_engine does, against the fp64 restatement tests/rollout_ref.py at the inputs of tests/rollout_cases.py.

Engines, all reachable in-process: "lane" (scratch NULL, the mean's window inside the LDS ring: a lane per path), "wave"
(scratch NULL, k one or more beyond the ring limit: a wave per path, append-only), "resub" (scratch given: re-substitution).
Mode 4 keeps no window, so its lane engine always fits and it has no in-process wave launch.

(a) the failure matrix: the jitter ladder, the substituted pivot and their precedence -- info exact on every engine, samples
    within the bound on the steps that are specified (all of them; after an exhausted ladder, steps 1 .. |info|).
(b) accuracy on healthy paths with different scalars per series, both sides of every ring limit, re-substitution at long H.
(c) addressing: samples, info and the scratch sit inside NaN / -999 guards (every launch of this module), the scratch is
    NaN-filled, ten bitwise repeats, misaligned == aligned bitwise, S = 1 with G = 3.
(d) volt_rollout_shared_f32 at G = 3.
The argument codes of both entries are in tests/test_host_cpu.py, the Python reporting in tests/test_rollout_reporting_host.py.

A real (unstubbed) failing run through rollout_series(solve="closed") is not posed: there rho = acc0, so base = 0 and every
pvar = 1/2 dx v^2 >= 0, every pivot dx v^2 >= 0 -- pred_vol[., 0] = 0 puts both exactly ON their decisions, which the margin
rule (0.5 J away) forbids, and nothing on that route moves them further.  report_info is run on the kernel's real codes instead.

Bound: |out - fp64| <= 2e-4 max(1, max |fp64 path|), the project's (tests/test_gpu_refshape.py); every case prints
"ROLLOUT <engine> <case> err/bound" before it asserts.  Largest ratios printed on the MI355X: failure matrix 0.012 (mode 4,
S = 70, H = 7; the same on the lane and the re-substitution engine), jitter = 0 0.001; healthy paths 0.074 (ewma, H = 300,
paths up to |y| = 64), 0.034 re-substitution at H = 257, <= 0.029 elsewhere, ring limits <= 0.010, S = 1 <= 0.002;
re-substitution against the default engine 0.15 / 0.05 / 0.25 of 5e-5 at H = 512 / 513 / 1024; shared kernel 0.034 (dewma,
k = 1, H = 65: all of it the input's amplification of the fp32 samples, tests/rollout_cases.py), 0.026 tewma k = 25,
<= 0.007 elsewhere.  info was exact on all three engines for all nine rows; the three copies of the ladder and the header's
description were found consistent."""
import functools

import numpy as np
import pytest
import torch

import rollout_cases as rc
import rollout_ref as rr

pytestmark = pytest.mark.gpu

PAD = 64                                  # guard floats on either side (256 B: the views stay 16-byte aligned)


def _guarded(n, fill, dtype, offset=0):
    buf = torch.full((n + 2 * PAD + 4,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD + offset:PAD + offset + n], PAD + offset


def _intact(buf, start, n, fill):
    rest = torch.cat((buf[:start], buf[start + n:]))
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


def _placed(a, offset):
    """The array on the device, ``offset`` floats past a 16-byte boundary."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    buf, view, _ = _guarded(t.numel(), 0.0, t.dtype, offset)
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == 4 * offset
    return buf, view


def launch(inp, engine, offset=0):
    """One launch of volt_rollout_bordered_f32.  Returns (samples [G,S,H], info [G,S]) as numpy; asserts the return code,
    the engine the shape selects, and that the guards around samples, info and the scratch are untouched."""
    from volt_amd import _lib
    L = _lib.lib()
    G, S, H = inp["pred_vol"].shape
    mode, k = inp["mean_mode"], inp["k"]
    assert rc.lane_ring_fits(mode, k) == (engine != "wave") or engine == "resub"
    assert engine != "wave" or H <= 256
    keep = []

    def dev(name, dtype):
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(inp[name], dtype=dtype))).cuda()
        keep.append(t)
        return t.data_ptr()
    f32, f64 = np.float32, np.float64
    pv_buf, pv = _placed(inp["pred_vol"], offset)
    z_buf, zz = _placed(inp["z"], offset)
    s_buf, smp, s0 = _guarded(G * S * H, float("nan"), torch.float32, offset)
    i_buf, info, i0 = _guarded(G * S, -999, torch.int32)
    scratch = None
    if engine == "resub":
        n = L.volt_rollout_scratch_bytes(G, S, H) // 4
        c_buf, scratch, c0 = _guarded(n, float("nan"), torch.float32)
    theta = inp["theta"]
    rc_ = L.volt_rollout_bordered_f32(
        dev("rho", f64), dev("tau", f64), dev("acc0", f64), dev("dx", f32), dev("hist_y", f32), dev("hist_e1", f32),
        dev("hist_e2", f32), dev("ema_prev", f32), dev("mr_latent", f32), dev("latent", f32), dev("w", f32), pv.data_ptr(),
        zz.data_ptr(), smp.data_ptr(), None if scratch is None else scratch.data_ptr(), info.data_ptr(), G, S, H, k, mode,
        int(theta is not None), float(theta or 0.0), float(inp["mr_theta"]), float(inp["jitter"]), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc_ == 0, rc_
    assert _intact(s_buf, s0, G * S * H, float("nan")), "a store outside samples"
    assert _intact(i_buf, i0, G * S, -999), "a store outside info"
    if scratch is not None:
        assert _intact(c_buf, c0, scratch.numel(), float("nan")), "a store outside the scratch"
    return smp.reshape(G, S, H).cpu().numpy().copy(), info.reshape(G, S).cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _failure(S, H, mode, theta, k, jitter=rc.J):
    inp, row = rc.failure_inputs(S, H, mode, theta, jitter=jitter, k=k)
    ref, info, tr = rc.run_ref(inp)
    mask = rr.compared_steps(info, H)
    assert rc.margins(tr, mask, jitter) >= 0.5 - 1e-5                   # a row that fails this is wrong: fix the row
    return inp, ref, info, mask


@functools.lru_cache(maxsize=None)
def _healthy(S, H, k, mode, theta):
    inp = rc.healthy_inputs(S, H, k, mode, theta)
    ref, info, tr = rc.run_ref(inp)
    assert (info == 0).all() and (tr["rung"] == -1).all() and min(tr["pvar"].min(), tr["d2"].min()) >= 0.5 * rc.J
    return inp, ref


def _ratio(out, ref, mask=None):
    """max over paths of err / bound on the compared steps."""
    d = np.abs(out.astype(np.float64) - ref)
    if mask is not None:
        assert np.isfinite(out[mask]).all()
        d = np.where(mask, d, 0.0)
    else:
        assert np.isfinite(out).all()
    return float((d.max(axis=-1, keepdims=True) / rc.path_bound(ref, mask)).max())


def _wave_k(mode):
    return {0: 582, 3: 582, 1: 296, 2: 198}[mode]


# ---------------------------------------------------------------------------------------------------------- (a)
FAILURE_LAUNCHES = [(e, m, t) for e in ("lane", "wave", "resub") for m, t in ((0, None), (2, None), (4, None), (0, 0.5))
                    if not (e == "wave" and m == 4)]      # mode 4 keeps no window: no in-process wave launch (module docstring)


@pytest.mark.parametrize("engine,mode,theta", FAILURE_LAUNCHES)
def test_failure_matrix(engine, mode, theta):
    """All nine rows (four series, delta = 4, 30, 150, 300 J) at S in {9, 70} and H in {8, 7} -- the lane engine's 16-byte and
    scalar instances: info is exactly the restatement's, the specified steps are within the bound."""
    from volt_amd import rollout_engine
    from volt_amd.gp import NotPSDError
    k = _wave_k(mode) if engine == "wave" else (1 if mode == 4 else 25)
    for S in (9, 70):
        for H in (8, 7):
            inp, ref, rinfo, mask = _failure(S, H, mode, theta, k)
            out, info = launch(inp, engine)
            r = _ratio(out, ref, mask)
            print(f"ROLLOUT {engine} failure_m{mode}{'t' if theta else ''}_S{S}_H{H} {r:.3f}")
            assert np.array_equal(info, rinfo), (S, H, info, rinfo)
            assert set(info.ravel()) == {-2, -1, 0, 1}
            assert r <= 1.0, (S, H, r)
    with pytest.raises(NotPSDError, match=r"\(first at horizon step 1\)"):
        rollout_engine.report_info(torch.as_tensor(info))


@pytest.mark.parametrize("engine", ["lane", "wave", "resub"])
def test_failure_matrix_without_jitter(engine):
    """jitter = 0: any pvar <= 0 is exhausted at once (the three rungs add nothing), the pivot floor is 1e-12."""
    inp, ref, rinfo, mask = _failure(9, 8, 0, None, _wave_k(0) if engine == "wave" else 25, 0.0)
    out, info = launch(inp, engine)
    r = _ratio(out, ref, mask)
    print(f"ROLLOUT {engine} failure_jitter0 {r:.3f}")
    assert np.array_equal(info, rinfo) and set(info.ravel()) == {-1, 0}
    assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("case", rc.HEALTHY_CASES, ids=[c[0] for c in rc.HEALTHY_CASES])
def test_healthy_paths_vs_fp64(case):
    name, mode, theta, S, H, k, engine = case
    inp, ref = _healthy(S, H, k, mode, theta)
    out, info = launch(inp, engine)
    r = _ratio(out, ref)
    print(f"ROLLOUT {engine} {name} {r:.3f}")
    assert not info.any()
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("H", [512, 513, 1024])
def test_resubstitution_at_long_horizons_vs_default_engine(H):
    """Beyond H = 300 the fp64 bound is not claimed; the two engines are held to each other at the project's 5e-5 of the
    paths' magnitude (rollout_engine.rollout_series, ``resubstitute``)."""
    inp = rc.healthy_inputs(3, H, 25, 0)
    a, ia = launch(inp, "lane")
    b, ib = launch(inp, "resub")
    assert not ia.any() and not ib.any() and np.isfinite(a).all() and np.isfinite(b).all()
    r = float(np.abs(a.astype(np.float64) - b).max() / (rc.ENGINE_BOUND * np.abs(a).max()))
    print(f"ROLLOUT resub-vs-lane m0_S3_H{H}_k25 {r:.3f}")
    assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("engine", ["lane", "wave", "resub"])
def test_ten_bitwise_repeats(engine):
    inp = _failure(70, 8, 0, None, _wave_k(0) if engine == "wave" else 25)[0]
    first = launch(inp, engine)
    for _ in range(9):
        again = launch(inp, engine)
        assert np.array_equal(first[0], again[0], equal_nan=True) and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("which", ["failure_S70_H8", "m3t_S65_H64_k2", "m1t_S65_H4_k64"])
def test_misaligned_launch_equals_aligned_bitwise(which):
    """pred_vol, z and samples one float past a 16-byte boundary with H % 4 == 0: the lane engine's scalar instance, which
    differs from the 16-byte one in loads and stores only."""
    if which.startswith("failure"):
        inp = _failure(70, 8, 0, None, 25)[0]
    else:
        _, mode, theta, S, H, k, _ = {c[0]: c for c in rc.HEALTHY_CASES}[which]
        inp = _healthy(S, H, k, mode, theta)[0]
    assert inp["pred_vol"].shape[-1] % 4 == 0
    a, ia = launch(inp, "lane")
    b, ib = launch(inp, "lane", offset=1)
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(ia, ib)


@pytest.mark.parametrize("engine", ["lane", "wave", "resub"])
def test_one_path_three_series(engine):
    """S = 1, G = 3: 63 idle lanes (3 idle waves) per series behind the only path."""
    k = _wave_k(0) if engine == "wave" else 25
    for H in (8, 7):
        inp, ref = _healthy(1, H, k, 0, 0.5)
        out, info = launch(inp, engine)
        r = _ratio(out, ref)
        print(f"ROLLOUT {engine} m0t_S1_H{H}_k{k} {r:.3f}")
        assert not info.any() and r <= 1.0


# ---------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("mode,S,H,k", rc.SHARED_CASES)
def test_shared_kernel_vs_fp64(mode, S, H, k):
    """volt_rollout_shared_f32 at G = 3 (the API only ever passes G = 1): e ~ N(0, 0.02^2), a NaN guard around samples."""
    from volt_amd import _lib
    hy, e1, e2, ema_prev, mrl, w, e = rc.shared_inputs(mode, S, H, k)
    ref = rr.shared_ref(hy, e1, e2, ema_prev, mrl, w, e, k, mode, 0.5)
    t = [torch.as_tensor(a).cuda() for a in (hy, e1, e2, ema_prev, mrl, w, e)]
    s_buf, smp, s0 = _guarded(3 * S * H, float("nan"), torch.float32)
    code = _lib.lib().volt_rollout_shared_f32(*(x.data_ptr() for x in t), smp.data_ptr(), 3, S, H, k, mode, 0.5,
                                              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0
    assert _intact(s_buf, s0, 3 * S * H, float("nan"))
    r = _ratio(smp.reshape(3, S, H).cpu().numpy(), ref)
    print(f"ROLLOUT shared m{mode}_S{S}_H{H}_k{k} {r:.3f}")
    assert r <= 1.0
