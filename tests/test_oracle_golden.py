"""Pin the CPU oracle to outputs of the reference's own code (tests/golden/*.npz, produced by
tests/golden/make_golden.py from /root/reference).  CPU-only."""
import numpy as np
import pytest

from oracle import volt_oracle as vo

FILL_TAGS = ["n7", "n64", "n257", "b3n50", "b2n130"]


@pytest.mark.parametrize("tag", FILL_TAGS)
def test_cumtrapz_bit_exact(golden, tag):
    g = golden("fill")
    vol, x = g[f"{tag}_vol"], g[f"{tag}_x"]
    V = vo.cumtrapz(vol * vol, x)
    assert V.dtype == np.float32
    assert np.array_equal(V, g[f"{tag}_V"])          # bit-exact (VolKernel.py:4-10)


@pytest.mark.parametrize("tag", FILL_TAGS)
def test_volatility_kernel_bit_exact(golden, tag):
    g = golden("fill")
    vol, x = g[f"{tag}_vol"], g[f"{tag}_x"]
    xx = x if vol.ndim == 1 else np.repeat(x[None], vol.shape[0], 0)
    K = vo.volatility_kernel(xx[..., None], vol[..., None])
    assert np.array_equal(K, g[f"{tag}_K"])          # VolKernel.py:18-42
    d = vo.volatility_kernel(xx[..., None], vol[..., None], diag=True)
    assert np.array_equal(d, g[f"{tag}_diag"])


def test_volatility_kernel_fp64_inherits_dtype(golden):
    g = golden("fill")
    K = vo.volatility_kernel(g["f64_x"][:, None], g["f64_vol"][:, None])
    assert K.dtype == np.float64
    np.testing.assert_allclose(K, g["f64_K"], rtol=1e-15, atol=0)


EW_TAGS = [("n60k5", 5), ("n60k25", 25), ("b3n40k7", 7), ("n300k100", 100)]


@pytest.mark.parametrize("tag,k", EW_TAGS)
def test_ewma_matches_reference(golden, tag, k):
    g = golden("ewma")
    y = g[f"{tag}_y"]
    out = vo.ewma(y, k)
    assert out.shape == g[f"{tag}_ewma"].shape       # length N+1 (EWMA.py:20-37)
    # conv1d summation order is unspecified: fp32 round-off only
    np.testing.assert_allclose(out, g[f"{tag}_ewma"], rtol=2e-6, atol=0)


@pytest.mark.parametrize("tag,k", EW_TAGS)
@pytest.mark.parametrize("cname", ["ewma", "dewma", "tewma", "meanrevert"])
def test_mean_classes_three_way_return(golden, tag, k, cname):
    g = golden("ewma")
    y, x = g[f"{tag}_y"], g[f"{tag}_x"]
    fn = {"ewma": vo.ewma_mean, "dewma": vo.dewma_mean, "tewma": vo.tewma_mean,
          "meanrevert": vo.meanrevert_mean}[cname]
    n = x.shape[0]
    for branch, xq in (("train", x), ("one", x[-1:] + np.float32(1 / 252.)), ("other", x[: n // 2])):
        ref = g[f"{tag}_{cname}_{branch}"]
        out = fn(xq, x, y, k)
        assert out.shape == ref.shape, (branch, out.shape, ref.shape)
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-6)


RO_TAGS = [("ewma", "ewma"), ("ewma_theta", "ewma"), ("dewma", "dewma"), ("tewma", "tewma"),
           ("ewma_n120", "ewma")]


@pytest.mark.parametrize("tag,mean", RO_TAGS)
def test_rollouts_match_reference_pathwise(golden, tag, mean):
    """Reference Rollouts (rollout_utils.py:57-93) with the same pred_vol and N(0,1) draws.
    fp32 dense Cholesky of the noise-free K (cond ~1e5..1e6 here) => compare at 2e-3 abs on
    log-prices ~2.3 (the reference's own LAPACK-vs-LAPACK reproducibility class)."""
    g = golden("rollouts")
    theta = float(g[f"{tag}_theta"])
    out = vo.rollouts(g[f"{tag}_train_x"], g[f"{tag}_train_y"], g[f"{tag}_test_x"],
                      np.log(g[f"{tag}_vol_path"]), g[f"{tag}_pred_vol"], g[f"{tag}_z"],
                      mean_name=mean, k=int(g[f"{tag}_k"]), theta=None if np.isnan(theta) else theta)
    ref = g[f"{tag}_samples"]
    assert out.shape == ref.shape
    np.testing.assert_allclose(out, ref, rtol=0, atol=2e-3)


def test_generate_prediction_multipoint(golden):
    g = golden("rollouts")
    tx, ty = g["gpm_train_x"], g["gpm_train_y"]
    c = np.float32(g["gpm_const"])
    out = vo.generate_prediction(tx, np.log(ty[1:]), np.log(g["gpm_vol_path"]), g["gpm_test_x"],
                                 g["gpm_pred_vol"], g["gpm_z"],
                                 lambda x: np.full((np.asarray(x).shape[0],), c, dtype=np.float32))
    assert out.shape == g["gpm_samples"].shape
    np.testing.assert_allclose(out, g["gpm_samples"], rtol=0, atol=2e-3)


# ----------------------------------------------------------------------------- (f)2: nonvol_rollouts
@pytest.mark.parametrize("tag,mean,kern", [("matern_ewma", "ewma", "matern"), ("rbf_dewma", "dewma", "rbf"),
                                           ("matern_tewma", "tewma", "matern")])
def test_nonvol_rollouts_match_reference_loop(golden, tag, mean, kern):
    """oracle.nonvol_rollouts vs the reference's own loop (rollout_utils.py:95-115) run with its EWMA mean classes and
    a dense fp64 predictive standing in for botorch's ``posterior`` (tests/golden/make_golden.py)."""
    d = golden("nonvol")
    ls, os_, noise, k = (float(d[f"{tag}_{n}"]) for n in ("ls", "os", "noise", "k"))
    kf = vo.matern_kernel if kern == "matern" else vo.rbf_kernel
    out = vo.nonvol_rollouts(d[f"{tag}_train_x"], d[f"{tag}_train_y"], d[f"{tag}_test_x"],
                             lambda a, b: kf(a, b, ls, os_), noise, d[f"{tag}_z"], mean_name=mean, k=int(k))
    assert np.abs(out - d[f"{tag}_samples"]).max() < 5e-5


def test_fp64_factor_and_solve_fixture(golden):
    """tests/golden/chol64.npz (reference's fp64 VolatilityKernel.forward + the ATen calls of rollout_utils.py:35-36):
    the oracle's fp64 kernel matrix factors and solves to the reference's own numbers."""
    g = golden("chol64")
    n = g["x"].shape[0]
    K = vo.volatility_kernel(g["x"], g["vol"])
    assert K.dtype == np.float64
    L, used = vo.psd_safe_cholesky(K, jitter=1e-4)
    assert used == 0.0
    Lref = np.zeros((n, n))
    Lref[np.tril_indices(n)] = g["L_packed"]
    np.testing.assert_allclose(L, Lref, rtol=0, atol=1e-10 * np.abs(Lref).max())
    sol = np.linalg.solve(L.T, np.linalg.solve(L, g["rhs"]))
    np.testing.assert_allclose(sol, g["sol"], rtol=0, atol=1e-8 * np.abs(g["sol"]).max())


@pytest.mark.parametrize("tag", ["n12d3", "n9d9", "n5d8", "n130d2"])
def test_last_dim_is_batch_matches_the_reference_code(golden, tag):
    """VolKernel.py:24-26,35-40 (``last_dim_is_batch``, with and without ``diag`` -- "TODO: check this" upstream, mirrored as
    written): fixtures from the reference's own forward (tests/golden/make_golden_ldb.py), bit-exact."""
    g = golden("fill_ldb")
    x, vol = g[f"{tag}_x"], g[f"{tag}_vol"]
    assert np.array_equal(vo.volatility_kernel_last_dim_is_batch(x, vol), g[f"{tag}_K"])
    assert np.array_equal(vo.volatility_kernel_last_dim_is_batch(x, vol, diag=True), g[f"{tag}_diag"])


# ----------------------------------------------------------------------------- reference shapes, fp64 (make_golden_refshape.py)
_EPS64 = np.finfo(np.float64).eps


def _refshape_tol(d, iset, out_max):
    """cond(K) * eps64 * max|path|, K the noise-free train block at the rollout's largest size (N + H - 1 points): the
    forward error of the fp64 solves the reference and the oracle both make, relative to the paths they produce.  The
    mean values are fp32 in both runs (the reference's FloatTensor casts); they are computed the same way, so they add
    nothing unless an fp32 rounding falls differently (a ~1e-9 chance per value)."""
    x = np.concatenate((d[f"{iset}_train_x"], d[f"{iset}_test_x"][:-1])).astype(np.float64)
    vol = np.concatenate((d[f"{iset}_vol"], d[f"{iset}_pred_vol"][0, :-1])).astype(np.float64)
    cond = np.linalg.cond(vo.volatility_kernel(x, vol))
    return cond * _EPS64 * max(1.0, out_max)


def _oracle_refshape(d, tag, **kw):
    iset = str(d[f"{tag}_set"])
    theta = float(d[f"{tag}_theta"])
    return vo.rollouts(d[f"{iset}_train_x"], d[f"{iset}_train_y"], d[f"{iset}_test_x"], np.log(d[f"{iset}_vol"]),
                       d[f"{iset}_pred_vol"], d[f"{iset}_z"], mean_name=str(d[f"{tag}_mean"]), k=int(d[f"{tag}_k"]),
                       theta=None if np.isnan(theta) else theta, dtype=np.float64, **kw)


@pytest.mark.parametrize("tag", ["tewma_k400", "meanrevert_k25", "ewma_k25_theta"])
def test_oracle_rollouts_match_reference_fp64(golden, tag):
    """oracle.rollouts in fp64 vs the reference's Rollouts run in fp64 with the same draws (tests/golden/rollouts_refshape.npz,
    N = 399, H = 100, S = 8; k > N - 1 at tewma k = 400), at cond(K) * eps64 * max|path| (~1e-8)."""
    d = golden("rollouts_refshape")
    out = _oracle_refshape(d, tag)
    ref = d[f"{tag}_s64"]
    assert out.dtype == np.float64 and out.shape == ref.shape
    tol = _refshape_tol(d, str(d[f"{tag}_set"]), float(np.abs(ref).max()))
    assert tol < 1e-7
    np.testing.assert_allclose(out, ref, rtol=0, atol=tol)


def test_meanrevert_latent_choice_cancels(golden):
    """The one negative control the GPU gate cannot see, pinned here: MeanRevertingEMAMean with its latent taken from the
    stacked series at every step instead of the one fixed at construction (EWMA.py:124).  The latent shifts every mean value
    of a step by the same theta * latent, and the predictive mean of the noise-free volatility kernel is
    y_last - m[N-1] + m_new (K^-1 u = e_last), so the shift cancels: the wrong variant matches the fp64 fixture too, up to
    how the shifted fp32 mean values round -- at most an fp32 ulp on each of m[N-1] and m_new per step, 2 H ulp(|y|) = 4.8e-5
    over H = 100 steps (measured 3.8e-6), under the GPU gate's 2e-4: harmless to the outputs, and invisible to it."""
    d = golden("rollouts_refshape")
    tag = "meanrevert_k25"
    ref = d[f"{tag}_s64"]
    out = _oracle_refshape(d, tag, stacked_latent=True)
    H = ref.shape[1]
    assert np.abs(out - ref).max() <= 2 * H * np.spacing(np.float32(np.abs(ref).max()))


@pytest.mark.parametrize("tag", ["voltron_T100_n3", "voltron_T1_n1", "magpie_k400_T1_n3"])
def test_oracle_generate_prediction_matches_model_twins_fp64(golden, tag):
    """The model-method twins (VoltronGP.py:62-95 with a linear mean, VoltMagpie.py:67-99 with EWMAMean at k > N) run in fp64:
    oracle.generate_prediction (default jitter, one column of draws at a time) at cond(K) * eps64 * max|path|."""
    t = golden("refshape_twins")
    T_, k = int(t[f"{tag}_T"]), int(t[f"{tag}_k"])
    x, ty, vol = t["in_train_x"], t["in_train_y"].astype(np.float64), t["in_vol"]
    ly = np.log(ty[1:])
    tx, pv = t["in_test_x"][:T_], t["in_pred_vol"][0, :T_]
    if tag.startswith("voltron"):
        w, b = float(t["lin_w"]), float(t["lin_b"])
        mfn = lambda q: w * np.asarray(q, dtype=np.float64).reshape(-1) + b
    else:
        mfn = lambda q: vo.ewma_mean(q, x, ly, k, dtype=np.float64)
    z = t[f"{tag}_z"].reshape(T_, -1)
    ref = t[f"{tag}_s64"].reshape(T_, -1)
    out = np.stack([vo.generate_prediction(x, ly, np.log(vol.astype(np.float64)), tx, pv[None], z[None, :, c:c + 1], mfn,
                                           jitter=None, dtype=np.float64)[0] for c in range(z.shape[1])], -1)
    xx = np.concatenate((x, tx)).astype(np.float64)
    tol = np.linalg.cond(vo.volatility_kernel(xx, np.concatenate((vol, pv)).astype(np.float64))) * _EPS64 * np.abs(ref).max()
    np.testing.assert_allclose(out, ref, rtol=0, atol=tol)


@pytest.mark.parametrize("k", [200, 400])
@pytest.mark.parametrize("cname", ["ewma", "dewma", "tewma", "meanrevert"])
def test_mean_functions_match_reference_fp64_beyond_n(golden, cname, k):
    """The oracle's mean functions with fp64 inputs and weights (the reference under torch's fp64 default dtype, its
    FloatTensor casts kept) at N = 399 with k > N / 2 and k > N, single and stacked [8, N+50]: one fp32 ulp (the same
    fp64 sums in another order may round the other way)."""
    t = golden("refshape_twins")
    fn = {"ewma": vo.ewma_mean, "dewma": vo.dewma_mean, "tewma": vo.tewma_mean, "meanrevert": vo.meanrevert_mean}[cname]
    x, y, xs, ys = (t[f"mc_{n}"].astype(np.float64) for n in ("x", "y", "xstack", "ystack"))
    kw = {"latent": y.mean()} if cname == "meanrevert" else {}
    q = {"train": (x, x, y), "one": (x[-1:] + 1 / 252., x, y), "other": (x[: x.shape[0] // 2], x, y),
         "btrain": (xs, xs, ys), "bone": (xs[-1:] + 1 / 252., xs, ys), "bother": (x, xs, ys)}
    for br, (xq, tx, ty) in q.items():
        ref = t[f"mc_{cname}_k{k}_{br}_64"]
        out = fn(xq, tx, ty, k, dtype=np.float64, **kw)
        assert out.dtype == np.float32 and out.shape == ref.shape, (br, out.shape, ref.shape)
        np.testing.assert_allclose(out, ref, rtol=0, atol=np.spacing(np.float32(4.0)), err_msg=br)
