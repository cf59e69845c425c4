"""tests/rollout_ref.py -- the fp64 restatement the GPU tests of csrc/rollout.hip are held to -- checked on the CPU by things
other than itself: the dense fp64 conditional of oracle/volt_oracle.py on healthy paths, a dense LAPACK forward substitution
on the paths whose pivots are substituted, the oracle's mean recursion for the shared-kernel rollouts; plus the margins of
the failure matrix and the negative controls at the inputs the GPU tests launch (tests/rollout_cases.py)."""
import numpy as np
import pytest
import scipy.linalg as sla

import rollout_cases as rc
import rollout_ref as rr
from oracle import volt_oracle as vo

MEANS = {"ewma": 0, "dewma": 1, "tewma": 2, "meanrevert": 3}


def _train_state(N, H, S, k, mean, seed):
    """A train block and the kernel-interface inputs derived from it in fp64 (rho, tau from dense solves)."""
    rng = np.random.default_rng(seed)
    f64 = np.float64
    train_x = np.arange(N, dtype=f64) / 252.0
    test_x = (N + np.arange(H, dtype=f64)) / 252.0
    train_y = np.exp(1.0 + np.cumsum(0.02 * rng.standard_normal(N + 1)))             # raw prices [N+1]
    log_vol = np.log(0.2) + 0.2 * rng.standard_normal(N)
    pred_vol = 0.15 + 0.15 * rng.random((S, H))
    z = rng.standard_normal((S, H))
    log_y = np.log(train_y[1:])
    dx = train_x[1] - train_x[0]
    v2 = np.exp(log_vol) ** 2
    wgt = np.full(N, dx)
    wgt[0] *= 0.5                                       # CumTrapz over the stacked path: only the first weight stays halved
    U = np.cumsum(wgt * v2)
    K = U[np.minimum.outer(np.arange(N), np.arange(N))]
    w = vo.ewma_weights(k, f64)
    mr_latent = np.float32(log_y.mean())
    m_tr = {"ewma": vo.ewma_mean, "dewma": vo.dewma_mean, "tewma": vo.tewma_mean}.get(mean)
    if m_tr is None:
        m_tr = vo.meanrevert_mean(train_x, train_x, log_y, k, 0.5, mr_latent, f64)
    else:
        m_tr = m_tr(train_x, train_x, log_y, k, f64)
    r_tr = log_y - m_tr.astype(f64)
    cf = sla.cho_factor(K, lower=True)
    rho = float(U @ sla.cho_solve(cf, U))
    tau = float(U @ sla.cho_solve(cf, r_tr))
    ema = vo.ewma(log_y, k, f64).astype(f64)                                          # [N+1], fp32 values
    ee = vo.ewma(ema, k, f64).astype(f64)[:-1]                                       # [N+1]

    def tail(a):
        a = a[:N]
        return (np.concatenate([np.repeat(a[:1], k - N), a]) if N < k else a[N - k:])[None]
    inp = dict(rho=[rho], tau=[tau], acc0=[U[-1]], dx=[dx], hist_y=tail(log_y), hist_e1=tail(ema), hist_e2=tail(ee),
               ema_prev=[ema[N - 1]], mr_latent=[mr_latent], latent=[np.log(train_y).mean()], w=w, pred_vol=pred_vol[None],
               z=z[None], k=k, mean_mode=MEANS[mean], theta=None, mr_theta=0.5, jitter=1e-4)
    return inp, (train_x, train_y, test_x, log_vol, pred_vol, z)


@pytest.mark.parametrize("theta", [None, 0.5])
@pytest.mark.parametrize("mean", sorted(MEANS))
@pytest.mark.parametrize("H", [1, 2, 24])
@pytest.mark.parametrize("N", [3, 64, 140])
def test_bordered_ref_matches_dense_oracle_on_healthy_paths(N, H, mean, theta):
    """bordered_ref against the dense fp64 conditional (oracle rollouts, dtype=fp64: an (N+idx)^2 factorisation per step and
    path) at 1e-9 of the path's magnitude; rho, tau, acc0 from dense fp64 solves on the train block (cond ~1e6).  The oracle
    keeps the reference's fp32 rounding of the mean module's values (EWMA.py:37): mean_dtype=fp32 rounds at the same places."""
    S, k = 3, 25
    inp, (train_x, train_y, test_x, log_vol, pred_vol, z) = _train_state(N, H, S, k, mean, 100 + N + H)
    inp["theta"] = theta
    ref = vo.rollouts(train_x, train_y, test_x, log_vol, pred_vol, z, mean_name=mean, k=k, theta=theta, mean_theta=0.5,
                      dtype=np.float64)
    out, info, tr = rc.run_ref(inp, mean_dtype=np.float32)
    assert (info == 0).all() and (tr["rung"] == -1).all() and not tr["subst"].any()
    err = float((np.abs(out[0] - ref).max(axis=-1) / np.maximum(1.0, np.abs(ref).max(axis=-1))).max())
    print(f"ROLLOUT_REF oracle N={N} H={H} {mean} theta={theta} max rel err {err:.3e}")
    assert err <= 1e-9
    # the collapse the issue describes: on a healthy path pvar = 1/2 dx v^2 and the pivot dx v^2, whatever came before
    dxv2 = inp["dx"][0] * pred_vol ** 2
    np.testing.assert_allclose(tr["pvar"][0], 0.5 * dxv2, rtol=0, atol=1e-9)
    np.testing.assert_allclose(tr["d2"][0], dxv2, rtol=0, atol=1e-9)
    # ... and the default (unrounded) means differ from the rounded ones by fp32 rounding of the level only
    out64, _, _ = rc.run_ref(inp)
    assert np.abs(out64 - out).max() <= 2e-5 * max(1.0, np.abs(out).max())


def _dense_check(inp, out, info, tr, g, s):
    """One path of bordered_ref against a dense fp64 forward substitution on S_s[a][b] = base_min(a,b) with the same
    substituted pivots: w_s, pvar, d2 and the sample of every compared step.  Returns the largest deviation."""
    H = out.shape[-1]
    dx = float(np.float32(inp["dx"][g]))
    pv = np.asarray(inp["pred_vol"][g, s], dtype=np.float64)
    zz = np.asarray(inp["z"][g, s], dtype=np.float64)
    tau = float(inp["tau"][g])
    base = float(inp["acc0"][g]) - float(inp["rho"][g]) + np.cumsum(dx * pv * pv)          # U_s - rho at appended point a
    Smat = base[np.minimum.outer(np.arange(H), np.arange(H))]
    floor = max(float(np.float32(inp["jitter"])), float(np.float32(1e-12)))
    last = -info[g, s] if info[g, s] < 0 else H
    L = np.zeros((H, H))
    r = np.zeros(H)                                                                     # r_s - tau 1
    worst = 0.0
    for a in range(last):
        w = sla.solve_triangular(L[:a, :a], Smat[:a, a], lower=True) if a else np.zeros(0)
        zs = sla.solve_triangular(L[:a, :a], r[:a], lower=True) if a else np.zeros(0)
        prev = base[a - 1] if a else float(inp["acc0"][g]) - float(inp["rho"][g])
        pvar = prev + 0.5 * dx * pv[a] ** 2 - w @ w
        d2 = Smat[a, a] - w @ w
        scale = max(1.0, abs(pvar), abs(d2), float(w @ w))
        if a:
            worst = max(worst, abs(w[-1] - tr["w"][g, s, a]) / max(1.0, abs(w[-1])))
        worst = max(worst, abs(pvar - tr["pvar"][g, s, a]) / scale, abs(d2 - tr["d2"][g, s, a]) / scale)
        pm = tau + w @ zs + tr["mstar"][g, s, a]
        if inp["theta"] is not None:
            pm = pm - float(np.float32(inp["theta"])) * (pm - float(inp["latent"][g]))
        used = pvar + tr["jit"][g, s, a] if tr["rung"][g, s, a] in (0, 1, 2) else (0.0 if tr["rung"][g, s, a] == 3 else pvar)
        smp = np.sqrt(used) * zz[a] + pm
        worst = max(worst, abs(smp - out[g, s, a]) / max(1.0, abs(smp)))
        assert (not d2 > 0) == bool(tr["subst"][g, s, a])
        L[a, :a] = w
        L[a, a] = np.sqrt(d2 if d2 > 0 else floor)
        r[a] = smp - tr["mstar"][g, s, a] - tau
    return worst


@pytest.mark.parametrize("mode,theta", [(0, None), (2, 0.5), (4, None)])
def test_failure_rows_match_the_table_and_dense_lapack(mode, theta):
    """The nine rows of the failure matrix: rung, pvar / J, d2 / J at the designed steps and info as tabled; every branch
    quantity of a compared step at least 0.5 J from its decision; and the restatement's w_s, pvar, d2 and samples step by step
    against scipy's triangular solves on the rebuilt per-sample matrix -- the ladder checked by something other than itself."""
    inp, row = rc.failure_inputs(9, 8, mode, theta)
    out, info, tr = rc.run_ref(inp)
    mask = rr.compared_steps(info, 8)
    seen = set()
    for g in range(row.shape[0]):
        for s in range(row.shape[1]):
            _, _, want_info, rungs, pvars, d2s = rc.FAILURE_ROWS[row[g, s]]
            seen.add(int(row[g, s]))
            assert info[g, s] == want_info, (row[g, s], info[g, s])
            for step in range(8):
                if mask[g, s, step]:
                    assert tr["rung"][g, s, step] == rungs.get(step, -1), (row[g, s], step)
            for step, v in pvars.items():
                assert tr["pvar"][g, s, step] / rc.J == pytest.approx(v, rel=1e-5), (row[g, s], step)
            for step, v in d2s.items():
                assert tr["d2"][g, s, step] / rc.J == pytest.approx(v, rel=1e-5), (row[g, s], step)
    assert seen == set(range(9))
    m = rc.margins(tr, mask, rc.J)
    print(f"ROLLOUT_REF failure matrix mode {mode}: smallest margin {m:.3f} J")
    assert m >= 0.5 - 1e-5
    worst = max(_dense_check(inp, out, info, tr, g, s) for g in range(row.shape[0]) for s in range(row.shape[1]))
    print(f"ROLLOUT_REF failure matrix mode {mode}: vs dense forward substitution {worst:.3e}")
    assert worst <= 1e-9
    # a path with an exhausted ladder really does diverge behind it (why nothing is asserted there)
    g, s = np.argwhere(row == 8)[0]
    assert np.abs(tr["w"][g, s]).max() > 1e6


def test_failure_matrix_margins_at_every_launch_shape():
    """The margin assertion for every failure-matrix launch of the GPU test (S, H, mode, theta, and the jitter = 0 launch, in
    which any pvar <= 0 is exhausted at once and a non-positive pivot never survives alone: d2 <= 0 implies pvar < 0)."""
    for S in (9, 70):
        for H in (8, 7):
            for mode, theta in ((0, None), (2, None), (4, None), (0, 0.5)):
                inp, _ = rc.failure_inputs(S, H, mode, theta)
                _, info, tr = rc.run_ref(inp)
                assert rc.margins(tr, rr.compared_steps(info, H), rc.J) >= 0.5 - 1e-5
                assert sorted(set(info.ravel())) == [-2, -1, 0, 1]
    inp, _ = rc.failure_inputs(9, 8, 0, None, jitter=0.0)
    _, info, tr = rc.run_ref(inp)
    assert rc.margins(tr, rr.compared_steps(info, 8), 0.0) >= 0.5 - 1e-5
    assert sorted(set(info.ravel())) == [-1, 0] and (tr["rung"][..., 0][info < 0] == 3).all()


def test_healthy_cases_stay_healthy_with_margin():
    """Every accuracy case: info 0, no ladder, no substitution, and every pvar and pivot at least 0.5 J above zero
    (the series with base = -2 J included: its first pvar is >= 12 J - 2 J)."""
    assert len(rc.HEALTHY_CASES) >= 20
    for name, mode, theta, S, H, k, engine in rc.HEALTHY_CASES:
        assert (engine == "wave") == (not rc.lane_ring_fits(mode, k)), name
        if k > 600 or H > 100:
            continue                                     # (same generator, same ranges: the long ones add nothing here)
        inp = rc.healthy_inputs(S, H, k, mode, theta)
        _, info, tr = rc.run_ref(inp)
        assert (info == 0).all() and (tr["rung"] == -1).all(), name
        assert min(tr["pvar"].min(), tr["d2"].min()) >= 0.5 * rc.J, name


@pytest.mark.parametrize("mean", sorted(MEANS))
def test_shared_ref_matches_the_oracle_mean_recursion(mean):
    """shared_ref against oracle nonvol_rollouts: with a white kernel k(a, b) = [a == b] and noise s2 the GP part of a path is
    e[idx] = sqrt(1) z[idx] exactly (no train point is correlated with a test point), so the oracle's samples are its mean
    recursion plus e.  The oracle rounds means and samples to fp32: 2e-6 relative."""
    N, H, S, k = 40, 12, 3, 20
    rng = np.random.default_rng(5)
    train_x = np.arange(N) / 252.0
    test_x = (N + np.arange(H)) / 252.0
    train_y = np.exp(1.0 + np.cumsum(0.02 * rng.standard_normal(N)))
    z = 0.02 * rng.standard_normal((S, H))
    kfun = lambda a, b: (np.asarray(a)[:, None] == np.asarray(b)[None, :]).astype(np.float64)
    ref = vo.nonvol_rollouts(train_x, train_y, test_x, kfun, 0.5, z, mean_name=mean, k=k, mean_theta=0.5)
    log_y = np.log(train_y.astype(np.float32)).astype(np.float32)
    w = vo.ewma_weights(k)
    ema = vo.ewma(log_y, k)
    ee = vo.ewma(ema, k)[:-1]
    out = rr.shared_ref(log_y[None, N - k:], ema[None, N - k:N], ee[None, N - k:N], [ema[N - 1]], [log_y.mean(dtype=np.float32)],
                        w, z[None], k, MEANS[mean], 0.5)
    err = float(np.abs(out[0] - ref).max() / np.abs(ref).max())
    print(f"ROLLOUT_REF shared {mean} max rel err {err:.3e}")
    assert err <= 2e-6


def test_shared_cases_are_well_conditioned():
    """Every shared-kernel case of the GPU test: rounding the stored samples to fp32 -- nothing else -- moves the restatement
    by at most 1/20 of the GPU bound; and the case that was taken out (tewma, k = 1, H = 300: a triple root at 1) by more than
    the whole bound, so no fp32 implementation could pass it."""
    def amplification(case):
        mode, S, H, k = case
        a = rc.shared_inputs(*case)
        r64 = rr.shared_ref(*a, k, mode, 0.5)
        r32 = rr.shared_ref(*a, k, mode, 0.5, sample_dtype=np.float32)
        return float((np.abs(r32 - r64).max(axis=-1, keepdims=True) / rc.path_bound(r64)).max())
    worst = {c: amplification(c) for c in rc.SHARED_CASES}
    print("ROLLOUT_REF shared conditioning (x bound)", {c: round(v, 4) for c, v in worst.items()})
    assert max(worst.values()) <= rc.SHARED_CONDITION
    assert {c[0] for c in rc.SHARED_CASES} == {0, 1, 2, 3} and {c[1] for c in rc.SHARED_CASES} == {1, 5, 9}
    assert {c[2] for c in rc.SHARED_CASES} == {1, 2, 65, 300} and {c[3] for c in rc.SHARED_CASES} == {1, 25, 300}
    assert amplification((2, 1, 300, 1)) > 1.0


def _moved(base, pert, mask=None):
    """How far a perturbed restatement lands from the true one, in units of the GPU tests' bound (max over paths)."""
    d = np.abs(pert - base)
    if mask is not None:
        d = np.where(mask, d, 0.0)
    return float((d.max(axis=-1, keepdims=True) / rc.path_bound(base, mask)).max())


def test_negative_controls_exceed_ten_times_the_gpu_bound():
    """Each deliberately wrong restatement, at the GPU tests' own inputs, lands more than 10 x the GPU tests' bound from the
    true one -- otherwise the inputs are too tame to see that mistake in a kernel."""
    moved = {}
    cases = {c[0]: c for c in rc.HEALTHY_CASES}

    def healthy(name, perturb):
        _, mode, theta, S, H, k, _ = cases[name]
        inp = rc.healthy_inputs(S, H, k, mode, theta)
        return _moved(rc.run_ref(inp)[0], rc.run_ref(inp, perturb=perturb)[0])
    moved["taps_shift"] = min(healthy(n, "taps_shift") for n in ("m2t_S5_H8_k25", "m3_S64_H63_k25", "m1_S64_H3_k25"))
    moved["kss_full_dx"] = min(healthy(n, "kss_full_dx") for n in ("m0t_S5_H2_k2", "m4_S5_H65"))
    moved["tau_prev_series"] = min(healthy(n, "tau_prev_series") for n in ("m0_S1_H1_k1", "m2_S130_H7_k65"))
    moved["theta_dropped"] = min(healthy(n, "theta_dropped") for n in ("m0t_S5_H2_k2", "m4t_S130_H100", "m3t_S65_H64_k2"))
    moved["ema_prev_stale"] = min(healthy(n, "ema_prev_stale") for n in ("m3_S64_H63_k25", "m3t_S65_H64_k2"))
    inp, _ = rc.failure_inputs(9, 8, 0)
    out, info, _ = rc.run_ref(inp)
    moved["ww_stale"] = _moved(out, rc.run_ref(inp, perturb="ww_stale")[0], rr.compared_steps(info, 8))
    print("ROLLOUT_REF controls (x bound)", {n: round(v, 1) for n, v in moved.items()})
    assert set(moved) == set(rr.PERTURBATIONS)
    for n, v in moved.items():
        assert v > 10.0, (n, v)
