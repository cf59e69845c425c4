"""Conditions on the references of tests/kron_cases.py (no GPU): in every regime the fp64 restatement is the dense fp64
definition, the floor of the fp32 interface lies an order of magnitude inside the project's fp32 bounds (so a kernel that
misses a gate there is the kernel's doing), and reconstruct_R inverts the prologue whatever basis the eigensolver picks."""
import numpy as np
import pytest
import torch

import kron_cases as kc
import kron_chain_ref as kref

TOL = 1e-10                       # the bound of tests/test_multitask_linear_host.py, relative to max(1, scale)
STEP_CASES = [(name, N, T, start) for name in kc.REGIMES for N, T in kc.SHAPES for start in (0, 1)]


@pytest.mark.parametrize("name,N,T,start", STEP_CASES)
def test_restatement_vs_dense_autograd_in_every_regime(name, N, T, start):
    """MLL and the five gradients of kref.kron_chain_ref against oracle_mll, scales max(1, .) as the fp64 gates.
    Measured: worst 3.6e-12 (covar_factor, noisy, 129 x 8, start = 0)."""
    r = kc.references(name, N, T, start, torch.float64)
    mll, g = kref.kron_chain_ref(kc.as_numpy(r["p"]), r["x"].numpy(), r["Y"].numpy())
    errs = kc.rel_errors(mll, g, *r["oracle"], floor_one=True)
    print(f"restatement {name} N={N} T={T} start={start}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("name,N,T,start", STEP_CASES)
def test_interface_floor_is_a_tenth_of_the_fp32_bounds(name, N, T, start):
    """The rounding of resid, sigma2, out and alpha to fp32 alone costs at most 1/10 of 5e-5 (MLL) and 2e-3 (each gradient).
    Measured: worst 5.3e-5 of the gradient's max (raw_var, noisy, 33 x 63, start = 0), a quarter of the 2e-4 asked here; the
    MLL's worst is 1.3e-7 (noisy, 65 x 3)."""
    r = kc.references(name, N, T, start, torch.float32)
    print(f"floor {name} N={N} T={T} start={start}: " + " ".join(f"{k}={v:.2e}" for k, v in r["floor"].items()))
    for k, e in r["floor"].items():
        assert e <= 0.1 * kc.F32_BOUND[k], (k, e)


@pytest.mark.parametrize("name", kc.REGIMES)
@pytest.mark.parametrize("N,T", [(1, 1), (5, 2), (65, 3), (33, 63), (7, 64)])
def test_reconstruct_r_inverts_the_prologue(name, N, T):
    p, x, Y = kc.case(name, N, T, 1)
    pn, xn, Yn = kc.as_numpy(p), x.numpy(), Y.numpy()
    pro = kref.prologue_ref(pn, xn, Yn)
    want = kc.residual_of(pn, xn, Yn)
    got = kc.reconstruct_R(pro["resid"], pro["lam"], pro["vol"], pro["Q"], pro["d"])
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    kc.eig_checks(pro["S"], pro["lam"], pro["Q"])
    if T > 1:
        # another basis of the same eigenspaces -- signs flipped everywhere, and in the tied regimes a rotation inside each
        # cluster -- with the resid that belongs to it: the same R
        Q2 = -pro["Q"]
        if name in ("scalar", "clusters"):
            rng = np.random.default_rng(T)
            for lo, hi in ((0, T // 2), (T // 2, T)) if name == "clusters" else ((0, T),):
                if hi - lo > 1:
                    rot, _ = np.linalg.qr(rng.standard_normal((hi - lo, hi - lo)))
                    Q2[:, lo:hi] = Q2[:, lo:hi] @ rot
        kc.eig_checks(pro["S"], pro["lam"], Q2)
        resid2 = ((want @ (Q2 / np.sqrt(pro["d"])[:, None])) / np.sqrt(pro["kappa"])[None, :]).T
        got2 = kc.reconstruct_R(resid2, pro["lam"], pro["vol"], Q2, pro["d"])
        assert np.abs(got2 - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_regimes_are_what_they_claim():
    """The spectra the GPU tests rely on."""
    T = 63
    lam = {}
    for name in kc.REGIMES:
        p, x, Y = kc.case(name, 33, T, 1)
        pro = kref.prologue_ref(kc.as_numpy(p), x.numpy(), Y.numpy())
        lam[name] = (pro["lam"], pro["kappa"])
    assert np.ptp(lam["scalar"][0]) == 0.0                                       # S = c I exactly
    cl = lam["clusters"][0]
    assert np.ptp(cl[:T // 2]) == 0.0 and np.ptp(cl[T // 2:]) == 0.0 and cl[0] < cl[-1] and len(set(cl)) == 2
    co = lam["correlated"][0]
    assert co[-1] / co[0] >= 5e3 and co[-2] / co[0] <= 2.0                       # one direction ~6e3 above the rest
    assert lam["noisy"][1][:-1].max() <= 1e-3 and lam["noisy"][1].max() <= 1e-2   # kappa << 1 (the last one carries |F|^2)
    assert lam["tiny_vol"][1].min() <= 2e-3
    p, _, _ = kc.case("linear_branch", 33, T, 1)
    assert float(p["raw_task_noises"][0]) > 20.0 and float(p["raw_var"][-1]) > 20.0   # ksoftplus's v > 20 branch, both uses
