"""GPU checks of the chain draws: volt_markov_draw_* / volt_vk_draw_* against the fp64 restatement of
tests/chain_draw_ref.py (validated against dense Cholesky in tests/test_chain_draw_host.py), their failure reports, the jitter
ladder around them, BMGP / MultitaskBMGP(posterior="chain"), the data model's draw="chain" routes, both drivers, and the memory
the two largest shapes take."""
import functools
import warnings

import numpy as np
import pytest
import torch

import chain_draw_ref as ref
import vk_forms_ref as vkref
from volt_amd.synthetic import rollout_inputs, sde_batch, sde_series

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
GATE = 1e-10                      # fp64 entries: of the draw's magnitude max |L z| (the restatement's own gate against dense Cholesky)
HS = (1, 2, 3, 4, 5, 63, 64, 65, 300, 1025)
SS = (1, 63, 64, 65, 130, 1000)
# every H with S = 65, every S with H = 5 and H = 65; G cycles through 1, 3, 65 (65 series only at the small shapes)
SHAPES = [((1, 3, 65)[i % 3] if H <= 65 else 3, 65, H) for i, H in enumerate(HS)] + \
         [((3, 1, 65)[i % 3] if S <= 130 else 3, S, H) for H in (5, 65) for i, S in enumerate(SS) if S != 65]
JITTERS = (0.0, 1e-6, 1e-2, 1e-8)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def in_nan_buffer(a, dtype):
    """The array as a strided view inside a NaN-filled device buffer (every other column, an offset of one row)."""
    a = np.asarray(a)
    buf = torch.full((a.shape[0] + 2,) + tuple(a.shape[1:-1]) + (2 * a.shape[-1] + 3,), float("nan"), dtype=dtype, device="cuda")
    view = buf[1:1 + a.shape[0], ..., 1:1 + 2 * a.shape[-1]:2]
    view.copy_(torch.as_tensor(a).to(dtype))
    assert not view.is_contiguous() or a.shape[-1] == 1
    return view


def behind(shape, dtype, fill):
    """(a contiguous view of ``shape`` at the front of a buffer, the 64 sentinel elements right behind it)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), fill, dtype=dtype, device="cuda")
    return buf[:n].view(*shape), buf[n:]


def sentinel_ok(tail, fill):
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


@functools.lru_cache(maxsize=None)
def markov_ref(G, S, H):
    mean, diag, off, z = ref.markov_case(G, S, H)
    z = f32(z)                                                     # the numbers both entries see
    jit = np.array([JITTERS[g % 4] for g in range(G)])
    want = np.stack([ref.markov_draw_ref(mean[g], diag[g], off[g], z[g], jit[g])[0] for g in range(G)])
    for a in (mean, diag, off, z, jit, want):
        a.setflags(write=False)
    return mean, diag, off, z, jit, want


@functools.lru_cache(maxsize=None)
def vk_ref(G, S, H, reps):
    pv, vl, vlr, dx, mean, z = ref.vk_case(G, S, H, reps)
    pv, z = f32(pv), f32(z)
    jit = np.array([JITTERS[g % 4] for g in range(G)])
    want = np.stack([ref.vk_draw_ref(pv[g], vl[g], vlr[g], dx[g], mean[g], z[g], jit[g], reps)[0] for g in range(G)])
    for a in (pv, vl, vlr, dx, mean, z, jit, want):
        a.setflags(write=False)
    return pv, vl, vlr, dx, mean, z, jit, want


def check_draw(got, want, mean, dtype, what, exp=False):
    """fp64 entries: GATE of the draw's magnitude; fp32 entries: + 2^-23 |ref|, the output's one rounding.  With exp: relative."""
    mag = np.abs(want - mean).max(axis=(-2, -1), keepdims=True)
    if exp:
        err, bound = np.abs(got / np.exp(want) - 1.0), GATE * mag + (EPS32 if dtype == torch.float32 else 0.0)
    else:
        err, bound = np.abs(got - want), GATE * mag + (EPS32 * np.abs(want) if dtype == torch.float32 else 0.0)
    assert np.isfinite(got).all()
    worst = float((err / bound).max())
    print(f"{what}: largest error / bound {worst:.3e}")
    assert worst <= 1.0, what


# ------------------------------------------------------------------------------------------------ 1: the kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("G,S,H", SHAPES)
def test_markov_draw_matches_the_restatement(G, S, H, dtype):
    from volt_amd import ops
    mean, diag, off, z, jit, want = markov_ref(G, S, H)
    args = [in_nan_buffer(a, torch.float64) for a in (mean, diag, off)] + [in_nan_buffer(z, dtype)]
    jd = in_nan_buffer(jit[None], torch.float64)[0]
    for exp in (False, True):
        out, out_tail = behind((G, S, H), dtype, float("nan"))
        info, info_tail = behind((G,), torch.int32, -77)
        o, i = ops.markov_draw(*args, jd, exp=exp, out=out, info=info)
        assert o is out and i is info and not info.any()
        first = out.clone()
        for _ in range(10):
            out.fill_(float("nan"))
            ops.markov_draw(*args, jd, exp=exp, out=out, info=info)
            assert torch.equal(out, first)
        assert sentinel_ok(out_tail, float("nan")) and sentinel_ok(info_tail, -77)
        check_draw(host(out), want, mean[:, None], dtype, f"markov {G} x {S} x {H} {dtype} exp = {exp}", exp)
    fresh, info = ops.markov_draw(*args, jd)
    assert torch.equal(fresh, ops.markov_draw(dev(mean, torch.float64), dev(diag, torch.float64), dev(off, torch.float64),
                                              dev(z, dtype), dev(jit, torch.float64))[0])          # the strided views changed nothing


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("G,S,H", SHAPES)
def test_vk_draw_matches_the_restatement(G, S, H, reps, dtype):
    from volt_amd import ops
    pv, vl, vlr, dx, mean, z, jit, want = vk_ref(G, S, H, reps)
    one = lambda a: in_nan_buffer(a[None], torch.float64)[0]
    args = (in_nan_buffer(pv, dtype), one(vl), one(vlr), one(dx), in_nan_buffer(mean, torch.float64), in_nan_buffer(z, dtype), one(jit))
    out, out_tail = behind((G, S * reps, H), dtype, float("nan"))
    info, info_tail = behind((G, S), torch.int32, -77)
    o, i = ops.vk_draw(*args, reps=reps, out=out, info=info)
    assert o is out and i is info and not info.any()
    first = out.clone()
    for _ in range(10):
        out.fill_(float("nan"))
        ops.vk_draw(*args, reps=reps, out=out, info=info)
        assert torch.equal(out, first)
    assert sentinel_ok(out_tail, float("nan")) and sentinel_ok(info_tail, -77)
    check_draw(host(out), want, mean[:, None], dtype, f"vk {G} x {S} x {H} reps = {reps} {dtype}")


def test_draws_replay_from_a_graph():
    from volt_amd import ops
    mean, diag, off, z, jit, want = markov_ref(3, 65, 65)
    a = [dev(t, torch.float64) for t in (mean, diag, off)] + [dev(z), dev(jit, torch.float64)]
    pv, vl, vlr, dx, vmean, vz, vjit, vwant = vk_ref(3, 65, 65, 1)
    b = [dev(pv)] + [dev(t, torch.float64) for t in (vl, vlr, dx, vmean)] + [dev(vz), dev(vjit, torch.float64)]
    out, info = torch.empty(3, 65, 65, device="cuda"), torch.empty(3, dtype=torch.int32, device="cuda")
    vout, vinfo = torch.empty(3, 65, 65, device="cuda"), torch.empty(3, 65, dtype=torch.int32, device="cuda")
    eager = ops.markov_draw(*a)[0], ops.vk_draw(*b)[0]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops.markov_draw(*a, out=out, info=info)
            ops.vk_draw(*b, out=vout, info=vinfo)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        out.fill_(float("nan"))
        vout.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(vout, eager[1]) and not info.any() and not vinfo.any()


def test_markov_mix_is_the_fp64_product_rounded_once():
    from volt_amd import ops
    rng = np.random.default_rng(7)
    for T, S, n in ((1, 1, 1), (3, 5, 7), (8, 17, 100), (64, 9, 33)):
        lz, V = rng.standard_normal((T, S, n)), f32(rng.standard_normal((T, T)))
        mean = f32(rng.standard_normal((n, T)))
        want = mean + np.einsum("tj,jsh->sht", V, lz)
        got = ops.markov_mix(dev(lz, torch.float64), dev(V), dev(mean))
        assert got.dtype == torch.float32 and tuple(got.shape) == (S, n, T)
        err = np.abs(host(got) - want)
        bound = 2.0 ** -24 * np.abs(want) * (1 + 1e-6) + 1e-14 * T          # one rounding of the output (+ the fp64 sum's own)
        assert (err <= bound).all(), (T, S, n, float((err / bound).max()))
        assert torch.equal(got, ops.markov_mix(dev(lz, torch.float64), dev(V), dev(mean)))
    with pytest.raises(ValueError):
        ops.markov_mix(dev(lz), dev(V), dev(mean))                           # fp32 lz
    with pytest.raises(ValueError):
        ops.markov_mix(dev(lz, torch.float64), dev(V)[:3], dev(mean))


def test_draws_validate_shapes():
    from volt_amd import ops
    a = torch.ones(2, 4, dtype=torch.float64, device="cuda")
    z = torch.zeros(2, 3, 4, device="cuda")
    with pytest.raises(ValueError):
        ops.markov_draw(a[:1], a, a, z)
    with pytest.raises(ValueError):
        ops.markov_draw(a, a, a, z[0])
    with pytest.raises(ValueError):
        ops.markov_draw(a, a, a, z, out=torch.empty(2, 3, 4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.vk_draw(z, 0.2, 1e-4, 1 / 252, a, z, reps=2)
    with pytest.raises(ValueError):
        ops.vk_draw(z, 0.2, 1e-4, 1 / 252, a[:, :3], z)


# ------------------------------------------------------------------------------------------------ 2: failures
def crafted_markov(H, i, rung=1e-6):
    """g = 1 and c_k = 0.01 (k + 1), except c_i = c_{i-1} - rung / 2 (i >= 1): at rung 0 step i has e_i = -rung / 2 and every
    step before it e = 0.01; at ``rung`` every e_k + rung is positive by at least rung / 2 (both checked on the restatement)."""
    assert i >= 1
    diag = 0.01 * (1.0 + np.arange(H))
    diag[i] = diag[i - 1] - 0.5 * rung
    off = diag.copy()
    c, g = ref.markov_cg(diag, off)
    t0 = ref.chain_pivots_ref(c, g, 0.0)
    assert len(t0) == i + 1 and (t0[:i] >= 0.5 * rung).all() and t0[i] <= -0.49 * rung
    t1 = ref.chain_pivots_ref(c, g, rung)
    assert len(t1) == H and (t1 >= 0.5 * rung).all()
    return diag, off


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("H,i", [(2, 1), (5, 4), (65, 31), (65, 32), (65, 64), (300, 170)])
def test_markov_draw_reports_the_first_failed_pivot(H, i, dtype):
    from volt_amd import ops
    S = 70
    rng = np.random.default_rng(H + i)
    good = ref.bm_posterior_diag_off(50, H, rng)
    bad_diag, bad_off = crafted_markov(H, i)
    diag, off = np.stack([good[2], bad_diag, good[2]]), np.stack([good[3], bad_off, good[3]])
    mean = np.stack([good[1]] * 3)
    z = f32(rng.standard_normal((3, S, H)))
    a = [dev(t, torch.float64) for t in (mean, diag, off)] + [dev(z, dtype)]
    out, info = ops.markov_draw(*a, 0.0)
    assert info.tolist() == [0, i + 1, 0]
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all()
    out6, info6 = ops.markov_draw(*a, 1e-6)
    assert not info6.any()
    want = ref.markov_draw_ref(mean[1], diag[1], off[1], z[1], 1e-6)[0]
    check_draw(host(out6[1:2]), want[None], mean[1][None, None], dtype, f"crafted H = {H} i = {i} at the first rung")
    # one bad series does not touch the others: series 0 at rung 0 is what it is alone
    alone, _ = ops.markov_draw(*(t[:1] for t in a), 0.0)
    assert torch.equal(alone[0], out[0])
    # a NaN in each input: diag / off / jitter fail the series (off[i] is read by step i + 1; the last one never), mean and z do not
    for k, name in enumerate(("mean", "diag", "off", "z")):
        b = [t.clone() for t in a]
        where = min(2, H - 1)
        b[k][0, ..., where] = float("nan")
        o, inf = ops.markov_draw(*b, 1e-6)
        code = {"mean": 0, "z": 0, "diag": where + 1, "off": where + 2 if where + 1 < H else 0}[name]
        assert inf.tolist() == [code, 0, 0], (name, inf.tolist())
        assert bool(torch.isnan(o[0]).all()) == (code != 0) and torch.isfinite(o[1:]).all()
        assert bool(torch.isnan(o[0]).any()) == (name != "off" or code != 0)       # (the last entry of off is never read)
    o, inf = ops.markov_draw(*a, torch.tensor([float("nan"), 1e-6, 1e-6], dtype=torch.float64, device="cuda"))
    assert inf.tolist() == [1, 0, 0] and torch.isnan(o[0]).all() and torch.equal(o[1:], out6[1:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("S,H,reps", [(70, 5, 1), (70, 65, 3), (130, 40, 1)])
def test_vk_draw_fails_chosen_paths_only(S, H, reps, dtype):
    """V_last - rho < 0 (what a jitter rung can leave) and a first test vol so small on the chosen paths that W_0 = -rung / 2:
    they fail at step 1 at rung 0 and pass at the rung; a NaN in pred_vol at step k fails at k + 1.  The other paths are
    bitwise what they are without the chosen ones."""
    from volt_amd import ops
    rung = 1e-6
    pv, vl, vlr, dx, mean, z = (np.array(a) for a in ref.vk_case(2, S, H, reps))
    pv, z = f32(pv), f32(z)
    vlr[:] = -5e-6                                                 # (every path of the case has dx pred_vol_0^2 > 1e-5)
    w0 = dx[0] * (0.5 if H == 1 else 1.0)
    chosen = np.arange(3, S, 17)
    base = [dev(pv, dtype)] + [dev(t, torch.float64) for t in (vl, vlr, dx, mean)] + [dev(z, dtype)]
    clean, info = ops.vk_draw(*base, 0.0, reps=reps)
    assert not info.any() and torch.isfinite(clean).all()
    pvb = pv.copy()
    pvb[1, chosen, 0] = np.sqrt((5e-6 - 0.5 * rung) / w0)
    W0 = ref.vk_W_ref(f32(pvb.astype(np.float32)) if dtype == torch.float32 else pvb, vl[:, None], vlr[:, None, None], dx[0])[1, chosen, 0]
    assert (W0 <= -0.4 * rung).all() and (W0 + rung >= 0.4 * rung).all()
    out, info = ops.vk_draw(dev(pvb, dtype), *base[1:], 0.0, reps=reps)
    want_info = np.zeros((2, S), dtype=np.int32)
    want_info[1, chosen] = 1
    assert np.array_equal(info.cpu().numpy(), want_info)
    rows = (chosen[:, None] * reps + np.arange(reps)).reshape(-1)
    keep = np.ones(S * reps, dtype=bool)
    keep[rows] = False
    assert torch.isnan(out[1, rows]).all() and torch.equal(out[0], clean[0]) and torch.equal(out[1, keep], clean[1, keep])
    out6, info6 = ops.vk_draw(dev(pvb, dtype), *base[1:], rung, reps=reps)
    assert not info6.any() and torch.isfinite(out6).all()
    # NaN in every input in turn
    k = min(2, H - 1)
    pvn = pv.copy()
    pvn[0, 5, k] = np.nan
    o, inf = ops.vk_draw(dev(pvn, dtype), *base[1:], 0.0, reps=reps)
    want_info[:] = 0
    want_info[0, 5] = k + 1
    assert np.array_equal(inf.cpu().numpy(), want_info) and torch.isnan(o[0, 5 * reps:6 * reps]).all()
    keep = np.ones(S * reps, dtype=bool)
    keep[5 * reps:6 * reps] = False
    assert torch.equal(o[0, keep], clean[0, keep]) and torch.equal(o[1], clean[1])
    for pos in (1, 2, 3, 6):                                        # vol_last, vlr, dx, jitter of series 1: its paths fail at step 1
        b = list(base) + [torch.zeros(2, dtype=torch.float64, device="cuda")]
        b[pos] = b[pos].clone()
        b[pos][1] = float("nan")
        o, inf = ops.vk_draw(*b, reps=reps)
        assert not inf[0].any() and bool((inf[1] == 1).all()) and torch.isnan(o[1]).all() and torch.equal(o[0], clean[0])
    for pos in (4, 5):                                              # mean, z: a NaN output, no failed pivot
        b = list(base)
        b[pos] = b[pos].clone()
        b[pos][1, ..., k] = float("nan")
        o, inf = ops.vk_draw(*b, 0.0, reps=reps)
        assert not inf.any() and torch.isnan(o[1]).any() and torch.equal(o[0], clean[0])


def test_safe_draw_applies_the_jitter_ladder():
    from volt_amd import gp
    H, i, S = 65, 32, 9
    diag, off = crafted_markov(H, i)
    rng = np.random.default_rng(3)
    mean, z = rng.standard_normal(H), f32(rng.standard_normal((1, S, H)))
    lazy = gp._MarkovCov(dev(diag, torch.float64), dev(off, torch.float64), dtype=torch.float32)
    with pytest.warns(gp.NumericalWarning, match="A not p.d., added jitter of 1.0e-06 to the diagonal"):
        got = host(lazy.draw(dev(mean, torch.float64)[None], dev(z)))
    C = gp._markov_cov(torch.tensor(diag), torch.tensor(off))
    L = torch.linalg.cholesky(C + 1e-6 * torch.eye(H, dtype=torch.float64)).numpy()
    want = mean + z[0] @ L.T
    check_draw(got, want[None], mean[None, None], torch.float32, "_safe_draw at the first rung against dense chol(C + 1e-6 I) z")
    lazy64 = gp._MarkovCov(dev(diag, torch.float64), dev(off, torch.float64), dtype=torch.float64)
    with pytest.warns(gp.NumericalWarning, match="A not p.d., added jitter of 1.0e-06 to the diagonal"):
        lazy64.draw(None, dev(z, torch.float64))                   # the fp64 model's ladder starts at 1e-8, 1e-7: the third rung passes
    hopeless = diag.copy()
    hopeless[i] = diag[i - 1] - 1.0
    with pytest.raises(gp.NotPSDError, match="after repeatedly adding jitter up to 1.0e-04"):
        gp._MarkovCov(dev(hopeless, torch.float64), dev(hopeless, torch.float64)).draw(None, dev(z))
    nan = diag.copy()
    nan[7] = np.nan
    with pytest.raises(gp.NanError) as err:
        gp._MarkovCov(dev(nan, torch.float64), dev(off, torch.float64)).draw(None, dev(z))
    assert not isinstance(err.value, gp.NotPSDError)


# ------------------------------------------------------------------------------------------------ 3: the vol forecaster
def _bmgp(x, y, posterior):
    from test_gpu_bm_post import _bmgp as build
    return build(x, y, torch.float32, posterior)


@pytest.mark.parametrize("N,T,H", [(120, 1, 1), (120, 3, 8), (399, 8, 100)])
def test_bmgp_chain_posterior_samples(N, T, H):
    """posterior="chain" beside "sweep" with the same base samples, ascending points (inside, on and beyond the grid): each
    sample's error against the fp64 restatement on the model's own fp64 forms is at most the sweep route's + 2^-23 |ref|; the
    two agree pathwise within 2e-3; mean, variance and covariance_matrix are the sweep route's bit for bit."""
    import bm_chain_ref as chain
    x = np.asarray(chain.grids(N)["uniform_dt"], dtype=np.float32)
    y = np.asarray(np.cumsum(np.random.default_rng(N + H).standard_normal((T, N)) * 0.05, axis=1) - 2.0, dtype=np.float32)
    y = y[0] if T == 1 else y
    xs = np.sort(np.concatenate([0.5 * (x[10:10 + H // 3] + x[11:11 + H // 3]), x[50:50 + H // 4],
                                 x[-1] + (1 + np.arange(H - H // 3 - H // 4)) / 252.0])).astype(np.float32)
    mc, _ = _bmgp(x, y, "chain")
    ms, _ = _bmgp(x, y, "sweep")
    pc, ps = mc(dev(xs)), ms(dev(xs))
    S = 33
    base = torch.randn(S, *pc.mean.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(H))
    lazy = pc.lazy_covariance_matrix
    diag, off = host(lazy.diag).reshape(T, H), host(lazy.off).reshape(T, H)
    mean64 = host(lazy.mean).reshape(T, H)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # (the dense fp32 factor may take a rung)
        a, b = pc.sample(base_samples=base), ps.sample(base_samples=base)
    assert a.shape == base.shape and a.dtype == torch.float32
    zz = host(base).reshape(S, T, H)
    want = np.stack([ref.markov_draw_ref(mean64[t], diag[t], off[t], zz[:, t], 0.0)[0] for t in range(T)], 1)
    ea, eb = np.abs(host(a).reshape(S, T, H) - want), np.abs(host(b).reshape(S, T, H) - want)
    bound = eb + EPS32 * np.abs(want)
    print(f"BMGP {N} x {T} H = {H}: max error chain {ea.max():.3e} sweep {eb.max():.3e}; largest chain / bound {(ea / bound).max():.3f}; "
          f"max |chain - sweep| {float((a - b).abs().max()):.3e} (bound 2e-3)")
    assert (ea <= bound).all() and float((a - b).abs().max()) <= 2e-3
    assert torch.equal(pc.mean, ps.mean) and torch.equal(pc.covariance_matrix, ps.covariance_matrix)
    assert torch.equal(pc.variance, ps.variance)
    draw = pc.sample(torch.Size((4,)))
    assert tuple(draw.shape) == (4,) + tuple(pc.mean.shape) and torch.isfinite(draw).all()


@pytest.mark.parametrize("N,T,H", [(120, 2, 1), (120, 3, 8), (399, 8, 100)])
def test_multitask_chain_posterior_samples(N, T, H):
    """MultitaskBMGP(posterior="chain") beside "sweep" with the same base samples: the chain's L_j z_j against the restatement
    on the model's own fp64 blocks, carried to the tasks in fp64, within the sweep route's own error + 2^-23 |ref|; pathwise
    2e-3; mean, variance and covariance bit for bit.  (T = 1 of the first shape is T = 2 here: a multitask model.)

    The directions reach the tasks through ops.markov_mix (fp64 sum, one rounding), not the dense route's fp32 GEMM: behind
    that GEMM the criterion cannot hold where T terms of size ~1 cancel (measured at (399, 8, 100): |ref| 0.081, the GEMM's own
    error on the restatement's L z 5.9e-8, against a bound of 1.5e-8 where the sweep route's error happened to be 5e-10)."""
    from test_gpu_multitask import make_case, model_params
    from volt_amd.gp import MultitaskGaussianLikelihood
    from volt_amd.models import MultitaskBMGP
    p, x, Y = make_case(N, T, 1, seed=N + T + H)
    xs = x[-1] + (torch.arange(H, dtype=torch.float32) + 1) / 252.
    if H >= 8:
        xs[:3] = torch.stack([0.5 * (x[5] + x[6]), x[17], 0.5 * (x[40] + x[41])])
    posts = {}
    for posterior in ("chain", "sweep"):
        lh = MultitaskGaussianLikelihood(num_tasks=T).cuda()
        m = MultitaskBMGP(x.cuda(), Y.cuda(), lh, solver="linear", posterior=posterior).cuda()
        with torch.no_grad():
            for k, prm in model_params(m, lh).items():
                prm.copy_(p[k])
        posts[posterior] = m.eval()(xs.cuda())
    pc, ps = posts["chain"], posts["sweep"]
    S = 17
    base = torch.randn(S, H, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(H))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = pc.sample(base_samples=base), ps.sample(base_samples=base)
    V, C = pc._blocks
    scale = host(C.scale)
    zz = host(base)
    lz = np.stack([ref.markov_draw_ref(np.zeros(H), scale[j] * host(C.diag)[j], scale[j] * host(C.off)[j], zz[:, :, j], 0.0)[0]
                   for j in range(T)], -1)                          # [S,H,T]: L_j z_j
    want = host(pc.mean) + lz @ host(V).T
    ea, eb = np.abs(host(a) - want), np.abs(host(b) - want)
    bound = eb + EPS32 * np.abs(want)
    print(f"multitask {N} x {T} H = {H}: max error chain {ea.max():.3e} sweep {eb.max():.3e}; largest chain / bound "
          f"{(ea / bound).max():.3f}; max |chain - sweep| {float((a - b).abs().max()):.3e} (bound 2e-3)")
    assert float((a - b).abs().max()) <= 2e-3
    assert torch.equal(pc.mean, ps.mean) and torch.equal(pc.variance, ps.variance)
    assert torch.equal(pc.covariance_matrix, ps.covariance_matrix)
    assert (ea <= bound).all(), float((ea / bound).max())


def test_shuffled_and_duplicated_points_on_the_chain_posterior():
    """Shuffled points: mean + P L_sorted P' z (the rule of gp._MarkovCov), against the restatement run over the sorted points.
    Duplicated points: the chain takes no rung or the first one, as a dense factor of the singular matrix does, and the twins
    move together."""
    import bm_chain_ref as chain
    from volt_amd import gp
    N, H, S = 120, 20, 9
    x = np.asarray(chain.grids(N)["uniform_dt"], dtype=np.float32)
    y = np.asarray(np.cumsum(np.random.default_rng(1).standard_normal(N) * 0.05) - 2.0, dtype=np.float32)
    xs_sorted = np.sort(np.concatenate([0.5 * (x[10:16] + x[11:17]), x[50:54], x[-1] + (1 + np.arange(10)) / 252.0])).astype(np.float32)
    perm = np.random.default_rng(2).permutation(H)
    xs = xs_sorted[perm]
    m, _ = _bmgp(x, y, "chain")
    post = m(dev(xs))
    lazy = post.lazy_covariance_matrix
    assert lazy.order is not None
    order = lazy.order.cpu().numpy()
    assert np.array_equal(xs[order], xs_sorted)
    base = torch.randn(S, H, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    got = host(post.sample(base_samples=base))
    z = host(base)
    mean_sorted = host(lazy.mean)[order]
    ys, _ = ref.markov_draw_ref(mean_sorted, host(lazy.diag), host(lazy.off), z[:, order], 0.0)
    want = np.empty_like(ys)
    want[:, order] = ys
    err = np.abs(got - want)
    assert (err <= EPS32 * np.abs(want) + GATE).all(), err.max()
    ms, _ = _bmgp(x, y, "sweep")
    assert torch.equal(post.covariance_matrix, ms(dev(xs)).covariance_matrix)
    # duplicates
    xd = xs_sorted.copy()
    xd[7] = xd[6]
    post = m(dev(xd))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        d = post.sample(base_samples=base)
    rungs = [str(w.message) for w in seen if issubclass(w.category, gp.NumericalWarning)]
    assert all("1.0e-06" in r for r in rungs), rungs
    assert torch.isfinite(d).all() and float((d[:, 7] - d[:, 6]).abs().max()) <= (1e-3 + 1e-4) * float(base.abs().max())
    # (the twin adds d z with d <= sqrt(1e-6); e / d against d at the rung and the outputs' roundings are within the 1e-4)


@pytest.mark.parametrize("H", [1, 20, 65])
@pytest.mark.parametrize("model", ["bmgp_f32", "bmgp_f64", "multitask"])
def test_sweep_is_the_chain_posterior_evaluated(model, H):
    """posterior="sweep" is posterior="chain" with its lazy covariance evaluated (one sweep, one gp._MarkovCov): the mean and the
    covariance are equal BITWISE, for BMGP at T x N = 3 x 65 in fp32 and fp64 and MultitaskBMGP at N x T = 65 x 3, the test
    points shuffled (inside, on and beyond the grid)."""
    N, T = 65, 3
    rng = np.random.default_rng(H)
    if model == "multitask":
        from test_gpu_multitask import make_case, model_params
        from volt_amd.gp import MultitaskGaussianLikelihood
        from volt_amd.models import MultitaskBMGP
        p, x, Y = make_case(N, T, 1, seed=N + T + H)
        x = x.numpy()
    else:
        import bm_chain_ref as chain
        from test_gpu_bm_post import _bmgp as build
        dtype = torch.float32 if model == "bmgp_f32" else torch.float64
        x = np.asarray(chain.grids(N)["uniform_dt"], dtype=np.float32)
        y = np.asarray(np.cumsum(rng.standard_normal((T, N)) * 0.05, axis=1) - 2.0, dtype=np.float32)
    xs = x[-1] + (1 + np.arange(H)) / 252.0
    if H >= 20:
        xs[:3] = [0.5 * (x[10] + x[11]), x[40], 0.5 * (x[50] + x[51])]
        xs = rng.permutation(xs)
        assert not (np.diff(xs) >= 0).all()
    xs = xs.astype(np.float32)
    posts = {}
    for posterior in ("chain", "sweep"):
        if model == "multitask":
            lh = MultitaskGaussianLikelihood(num_tasks=T).cuda()
            m = MultitaskBMGP(dev(x), Y.cuda(), lh, solver="linear", posterior=posterior).cuda()
            with torch.no_grad():
                for k, prm in model_params(m, lh).items():
                    prm.copy_(p[k])
            posts[posterior] = m.eval()(dev(xs))
        else:
            posts[posterior] = build(x, y, dtype, posterior)[0](dev(xs, dtype))
    pc, ps = posts["chain"], posts["sweep"]
    assert pc.mean.dtype == ps.mean.dtype and torch.isfinite(ps.mean).all()
    assert torch.equal(ps.mean, pc.mean)
    assert torch.equal(ps.covariance_matrix, pc.covariance_matrix)
    if model != "multitask":
        from volt_amd import gp
        assert isinstance(pc.lazy_covariance_matrix, gp._MarkovCov) and (pc.lazy_covariance_matrix.order is None) == (H == 1)
        assert tuple(ps.covariance_matrix.shape) == (T, H, H) and ps.mean.dtype == dtype


# ------------------------------------------------------------------------------------------------ 4: the data model
@pytest.mark.parametrize("N,T,S", vkref.DRAW_SHAPES)
def test_chain_draw_is_at_least_as_accurate_as_the_factor_draw(N, T, S):
    """_posterior_draw_linear(draw="chain") beside draw="factor" and the dense fp32 draw on the same inputs, against the fp64
    oracle: per output the chain's error is at most the factor route's + 2^-23 |ref| (the output's one rounding)."""
    from test_gpu_predict_linear import _draw_args
    from volt_amd.kernels import VolatilityKernel
    from volt_amd.rollout_utils import _posterior_draw, _posterior_draw_linear
    x, y, vol, test_x, pv, z, want = vkref.draw_case(N, T, S)
    args = _draw_args(x, y, vol, test_x, pv, z)
    k = VolatilityKernel().cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dense = host(_posterior_draw(k, *args, 1e-4).squeeze(-1))
        factor = host(_posterior_draw_linear(k, *args, 1e-4).squeeze(-1))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = _posterior_draw_linear(k, *args, 1e-4, draw="chain")
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, T, 1)
    e_c, e_f, e_d = (np.abs(host(t).reshape(S, T) - want) for t in (got, torch.as_tensor(factor), torch.as_tensor(dense)))
    bound = e_f + EPS32 * np.abs(want)
    print(f"draw N = {N} T = {T} S = {S}: max error chain {e_c.max():.3e} factor {e_f.max():.3e} dense fp32 {e_d.max():.3e}; "
          f"largest chain / bound {(e_c / bound).max():.3f}")
    assert (e_c <= bound).all() and e_c.max() <= 2e-3
    # per-sample histories (S grids in one launch): sample 0 to the bit
    a = _draw_args(x, y, vol, test_x, pv, z, per_sample=True)
    fv = a[1].clone()
    fv[1:, 0] *= 1.0 + 2.0 ** -20
    per = _posterior_draw_linear(k, a[0].unsqueeze(0).repeat(S, 1), fv, *a[2:], 1e-4, draw="chain")
    assert torch.equal(per[0], got[0]) and (np.abs(host(per).reshape(S, T) - want) <= bound + 1e-9).all()


def test_chain_draw_with_three_columns_and_theta():
    """n = 3 columns of z (`reps`) and the mean reversion: every column against the fp64 oracle run on that column, within the
    factor route's own error + 2^-23 |ref|."""
    from oracle import volt_oracle as vo
    from test_gpu_predict_linear import _draw_args
    from volt_amd.kernels import VolatilityKernel
    from volt_amd.rollout_utils import _posterior_draw_linear
    N, T, S = 90, 6, 5
    x, y, vol, test_x, pv, z, _ = vkref.draw_case(N, T, S)
    z3 = np.asarray(np.random.default_rng(6).standard_normal((S, T, 3)), dtype=np.float32)
    args = list(_draw_args(x, y, vol, test_x, pv, z))
    args[-1] = dev(z3)
    lat = torch.tensor(2.25, device="cuda")
    k = VolatilityKernel().cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        factor = host(_posterior_draw_linear(k, *args, 1e-4, lat, 0.3))
    got = host(_posterior_draw_linear(k, *args, 1e-4, lat, 0.3, draw="chain"))
    assert got.shape == (S, T, 3)
    for c in range(3):
        want = vo.generate_prediction(x, y, np.log(vol.astype(np.float64)), test_x, pv, z3[:, :, c:c + 1], vkref.linear_mean,
                                      dtype=np.float64, latent_mean=2.25, theta=0.3)
        e_c, e_f = np.abs(got[:, :, c] - want), np.abs(factor[:, :, c] - want)
        print(f"column {c}: max error chain {e_c.max():.3e} factor {e_f.max():.3e}")
        assert (e_c <= e_f + EPS32 * np.abs(want)).all()


@pytest.mark.parametrize("cls_name", ["VoltMagpie", "VoltronGP"])
def test_models_with_the_chain_draw_match_the_factor_draw(cls_name):
    """Every prediction method and Rollouts on the dense engine: predict_draw="chain" against "factor" (both predict_solver=
    "linear") on identical draws within 2e-3; Rollouts leaves both models in the same mutated state."""
    from test_gpu_predict_linear import _model
    from volt_amd import models
    from volt_amd.rollout_utils import GeneratePrediction, Rollouts
    cls = getattr(models, cls_name)
    n, H, S = 90, 6, 5
    F, vol = sde_series(n, 31)
    tx = torch.arange(n, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    prices, y, vp = dev(F), dev(F)[1:].log(), dev(vol)
    pv = dev(np.full(H, vol[-1], dtype=np.float32))
    g = torch.Generator().manual_seed(5)
    pred_vol = (vp[-1].log() + 0.05 * torch.randn(S, H, generator=g).cumsum(-1).cuda()).exp()
    z = torch.randn(S, H, generator=g).cuda()
    Hm = H if cls_name == "VoltronGP" else 1
    mx = test_x[:Hm]
    outs, states = {}, {}
    for draw in ("chain", "factor"):
        m = _model(cls, tx, y, vp, "linear", predict_draw=draw)
        assert m.predict_draw == draw
        torch.manual_seed(11)
        outs[draw, "method"] = m.GeneratePrediction(mx, pv[:Hm], 3)
        torch.manual_seed(11)
        outs[draw, "method1"] = m.GeneratePrediction(test_x[:1], pv[:1])
        m.vol_model.eval()
        torch.manual_seed(12)
        outs[draw, "sample"] = m.SamplePrediction(mx, n_sample=2)
        torch.manual_seed(12)
        outs[draw, "mean"] = m.MeanPrediction(mx, n_sample=2)
        fargs = (tx, prices, mx, pred_vol[:, :Hm], m)
        outs[draw, "function"] = GeneratePrediction(*fargs, z=z[:, :Hm].unsqueeze(-1))
        outs[draw, "override"] = GeneratePrediction(*fargs, z=z[:, :Hm].unsqueeze(-1), draw="factor" if draw == "chain" else "chain")
        m2 = _model(cls, tx, y, vp, "linear", predict_draw=draw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs[draw, "rollouts"] = Rollouts(tx, prices, test_x, m2, nsample=S, pred_vol=pred_vol, z=z, engine="dense")
        states[draw] = (m2.train_x, m2.train_y, m2.log_vol_path, m2.mean_module.train_x, m2.mean_module.train_y)
    for key in ("method", "method1", "sample", "mean", "function", "rollouts"):
        a, b = outs["chain", key], outs["factor", key]
        assert torch.isfinite(a).all() and a.shape == b.shape
        err = float((a - b).abs().max())
        print(f"{cls_name} {key}: max |chain - factor| = {err:.3e} (bound 2e-3)")
        assert err < 2e-3, key
    assert torch.equal(outs["chain", "override"], outs["factor", "function"])
    assert torch.equal(outs["factor", "override"], outs["chain", "function"])
    for a, b in zip(states["chain"], states["factor"]):
        assert a.shape == b.shape and float((a - b).abs().max()) < 2e-3
    assert torch.equal(states["chain"][0], states["factor"][0]) and torch.equal(states["chain"][2], states["factor"][2])
    with pytest.raises(ValueError, match="solver='linear'"):
        GeneratePrediction(tx, prices, mx, pred_vol[:, :Hm], _model(cls, tx, y, vp, "dense"), draw="chain")


# ------------------------------------------------------------------------------------------------ 5: the drivers
def _count(monkeypatch, name):
    from volt_amd import ops
    calls, real = [], getattr(ops, name)

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, spy)
    return calls


def test_volt_forecast_with_the_chain_options(monkeypatch):
    """Volt(vol_posterior="chain", predict_draw="chain") beside "sweep" / "factor", built, trained and forecast under the same
    seeds on the dense engine (the one predict_draw reaches): 2e-4, the driver's bound; the vol paths came from the chain."""
    from volt_amd.models.Volt import Volt
    n, H, S = 130, 6, 8
    F, vol = sde_series(n, 5)
    tx = torch.arange(n + 1, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    calls = _count(monkeypatch, "markov_draw")
    outs = {}
    for vp, pd in (("chain", "chain"), ("sweep", "factor")):
        torch.manual_seed(3)
        m = Volt(tx, dev(F).log(), mean="ewma", vol_path=dev(vol), k=10, vol_solver="linear", predict_solver="linear",
                 vol_posterior=vp, predict_draw=pd)
        torch.manual_seed(5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.Train(gpcv_iters=5, vol_mod_iters=5, data_mod_iters=4)
        assert m.vol_model.posterior == vp and m.predict_draw == pd
        torch.manual_seed(11)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs[vp] = m.Forecast(test_x, nsample=S, engine="dense")
        assert len(calls) == 1                                      # one launch for the S vol paths, none on the sweep route
    d = float((outs["chain"] - outs["sweep"]).abs().max())
    print(f"Volt.Forecast: max |chain - sweep / factor| = {d:.3e} (bound 2e-4)")
    assert tuple(outs["chain"].shape) == (S, H) and torch.isfinite(outs["chain"]).all() and d <= 2e-4


@pytest.mark.parametrize("mean,multitask", [("ewma", False), ("constant", False), ("constant", True)])
def test_stocks_driver_with_the_chain_options(mean, multitask, monkeypatch):
    """Both branches of the stocks driver (Rollouts: ewma; standard mean: constant) with vol_posterior="chain",
    predict_draw="chain" beside "sweep" / "factor" under the same generator: 2e-4.  The standard-mean branch is ONE vk_draw
    launch for all tickers."""
    from volt_amd.forecast import GenerateStockPredictionsBatch
    B, ntrain, H, S = 3, 130, 4, 5
    _, F, _ = sde_batch(B, ntrain + 5, seed=77)
    closes = torch.as_tensor(np.asarray(F)).cuda()
    vk_calls, mk_calls = _count(monkeypatch, "vk_draw"), _count(monkeypatch, "markov_draw")
    outs = {}
    for vp, pd in (("chain", "chain"), ("sweep", "factor")):
        g = torch.Generator(device="cuda").manual_seed(1)
        torch.manual_seed(1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs[vp] = GenerateStockPredictionsBatch(["AAA", "BBB", "CCC"], closes, forecast_horizon=H, train_iters=3, nsample=S,
                                                     ntrain=ntrain, mean=mean, k=10, ntimes=1, vol_iters=4, generator=g,
                                                     vol_solver="linear", predict_solver="linear", multitask_vol=multitask,
                                                     vol_posterior=vp, predict_draw=pd)
        assert len(mk_calls) == 1 and len(vk_calls) == (1 if mean == "constant" else 0)
    d = float((outs["chain"] - outs["sweep"]).abs().max())
    print(f"stocks driver {mean} multitask = {multitask}: max |chain - sweep / factor| = {d:.3e} (bound 2e-4)")
    assert tuple(outs["chain"].shape) == (B, S, H) and torch.isfinite(outs["chain"]).all() and d <= 2e-4


# ------------------------------------------------------------------------------------------------ 6: memory
def _peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    return res, torch.cuda.max_memory_allocated() - base


def test_standard_mean_chain_at_2_x_4096_x_1024_holds_nothing_but_its_result():
    """B = 2, N = 399, S = 4096, H = 1024: the peak above the inputs and the [B,S,H] result is <= 8 MB -- the factor route's
    H x H blocks would be 34 GB and its ``tail`` 67 MB."""
    from volt_amd.forecast import _standard_mean_prediction_linear
    B, N, S, H = 2, 399, 4096, 1024
    x, F, vol = sde_batch(B, N, seed=3)
    tx = torch.arange(N, device="cuda") / 252.
    test_x = torch.arange(H, device="cuda") / 252. + tx[-1] + tx[1]
    g = torch.Generator(device="cuda").manual_seed(2)
    pred_vol = (dev(vol)[:, -1:, None].log() + 0.01 * torch.randn(B, S, H, device="cuda", generator=g).cumsum(-1)).exp()
    z = torch.randn(B, S, H, device="cuda", generator=g)
    resid = dev(F)[:, 1:].log() - 4.0
    m_te = torch.full((B, H), 4.0, device="cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out, grown = _peak_growth(lambda: _standard_mean_prediction_linear(tx, resid, m_te, dev(vol), test_x, pred_vol, z, draw="chain"))
    extra = grown - out.numel() * out.element_size()
    print(f"standard-mean chain 2 x 4096 x 1024: peak above inputs and result {extra / 2 ** 20:.2f} MB (bound 8 MB)")
    assert tuple(out.shape) == (B, S, H) and out.dtype == torch.float32 and torch.isfinite(out).all()
    assert extra <= 8 * 2 ** 20, extra
    # and it is the factor route's draw where that one fits: the first 3 paths at H = 64
    small = _standard_mean_prediction_linear(tx, resid, m_te[:, :64], dev(vol), test_x[:64], pred_vol[:, :3, :64].contiguous(),
                                             z[:, :3, :64].contiguous(), draw="chain")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fact = _standard_mean_prediction_linear(tx, resid, m_te[:, :64], dev(vol), test_x[:64], pred_vol[:, :3, :64].contiguous(),
                                                z[:, :3, :64].contiguous())
    assert float((small - fact).abs().max()) <= 2e-3


def test_bmgp_chain_sample_4096_at_h_1024_holds_nothing_but_its_result():
    """BMGP(posterior="chain").sample([4096]) at H = 1024: <= 8 MB above the base samples and the result (the dense route's
    H x H covariance and factor alone are 8 MB, its fp64 assembly 25 MB)."""
    import bm_chain_ref as chain
    N, H, S = 399, 1024, 4096
    x = np.asarray(chain.grids(N)["uniform_dt"], dtype=np.float32)
    y = np.asarray(np.cumsum(np.random.default_rng(9).standard_normal(N) * 0.05) - 2.0, dtype=np.float32)
    m, _ = _bmgp(x, y, "chain")
    xs = dev(x[-1] + (1 + np.arange(H)) / 252.0)
    post = m(xs)
    base = torch.randn(S, H, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out, grown = _peak_growth(lambda: post.sample(base_samples=base))
    extra = grown - out.numel() * out.element_size()
    print(f"BMGP chain sample 4096 x 1024: peak above base samples and result {extra / 2 ** 20:.2f} MB (bound 8 MB)")
    assert tuple(out.shape) == (S, H) and torch.isfinite(out).all() and extra <= 8 * 2 ** 20, extra
    var = out.double().var(0)
    want = post.variance.double()
    assert float((var / want - 1).abs().max()) < 0.2             # 4096 draws: the sample variance within 5 sigma of the posterior's
