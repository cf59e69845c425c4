"""Prediction from the Markov GPCV away from its grid (csrc/markov_predict.hip), without a device:
  * the fp64 restatement (tests/markov_predict_ref.py) against the dense definition A = K*u Kuu^-1, mean mu + A (m - mu),
    C = A P^-1 A' + (K** - A Kuu A') -- mean, var_q, var_p and the draw's chain and bridge maps each on their own;
  * at every input the GPU tests run (PR.GPU_CASES, one list for both files): the same comparison, four negative controls, each a
    single wrong term, which must miss the GPU bound by more than 10 x wherever they can act, and the fp32 output within half of
    the GPU bound;
  * the C entry points' argument codes, the workspace formula, the exported names, a cross-compile of the new file without
    scratch, spills or atomics, and the unchanged refusals of the "dense" and "linear" families."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import markov_predict_ref as PR  # noqa: E402

BOUND = 1e-10                      # of each quantity's scale: the project's standing bound for restatements


def _errors(x, xs, v, mu, m, rho, gamma, variant=None, dense=None):
    """Largest error / scale of (mean, var_q, var_p, Fk Fk', Fb Fb') against the dense definition, in the caller's order."""
    mean_d, Cq, Cp = PR.dense_definition(x, xs, v, mu, m, rho, gamma) if dense is None else dense
    pl = PR.plan(x, xs, v, mu, m, rho, gamma, variant=variant)
    Fk, Fb = PR.draw_maps(pl)
    inv = np.empty_like(pl["order"])
    inv[pl["order"]] = np.arange(pl["H"])
    P = np.ix_(inv, inv)
    sc = max(np.abs(Cq).max(), np.abs(Cp).max(), 1e-300)
    return {"mean": np.abs(PR.unsort(pl, pl["mean"]) - mean_d).max() / max(1.0, np.abs(mean_d).max()),
            "var_q": np.abs(PR.unsort(pl, pl["var_q"]) - np.diag(Cq)).max() / sc,
            "var_p": np.abs(PR.unsort(pl, pl["var_p"]) - np.diag(Cp)).max() / sc,
            "chain": np.abs((Fk @ Fk.T)[P] - Cq).max() / sc,
            "bridge": np.abs((Fb @ Fb.T)[P] - Cp).max() / sc,
            "cross": np.abs(Fk * Fb).max()}


@pytest.mark.parametrize("regime", PR.REGIMES)
def test_restatement_matches_the_dense_definition(regime):
    worst = {}
    for N, x0, v in PR.HOST_SHAPES:
        x = PR.make_grid(N, x0)
        m, rho, gamma, mu = PR.make_params(x, v, regime)
        for family in PR.FAMILIES:
            xs = PR.make_points(x, family)
            err = _errors(x, xs, v, mu[0], m[0], rho[0], gamma[0])
            for k, e in err.items():
                if e > worst.get(k, (-1.0,))[0]:
                    worst[k] = (e, N, x0, v, family)
    for k, w in worst.items():
        print(f"{regime:8s} {k:7s} largest error / scale {w[0]:.2e} at N = {w[1]}, x0 = {w[2]:.4f}, v = {w[3]}, {w[4]}")
    assert worst["cross"][0] == 0.0                                    # the chain and the bridge steps use disjoint base samples
    for k in ("mean", "var_q", "var_p", "chain", "bridge"):
        assert worst[k][0] <= BOUND, (k, worst[k])


def test_plan_shape_and_copies():
    """E <= 3 H + 1; a duplicated point and a point on its right knot copy their anchor (0, 1, 0), never 0 / 0."""
    for N, x0, v in PR.HOST_SHAPES:
        x = PR.make_grid(N, x0)
        m, rho, gamma, mu = PR.make_params(x, v, "random")
        for family in PR.FAMILIES:
            xs = PR.make_points(x, family)
            pl = PR.plan(x, xs, v, mu[0], m[0], rho[0], gamma[0])
            assert len(pl["steps"]) <= 3 * pl["H"] + 1
            assert all(np.isfinite([a, b, c]).all() for _, _, a, b, c in pl["steps"])
            xo = xs[pl["order"]]
            Fk, Fb = PR.draw_maps(pl)
            for h in range(pl["H"] - 1):
                if xo[h] == xo[h + 1]:
                    assert np.array_equal(Fk[h], Fk[h + 1]) and np.array_equal(Fb[h], Fb[h + 1])
            if family == "same":                                       # on the grid: q(u) itself
                assert np.array_equal(pl["mean"], m[0]) and np.all(pl["var_p"] == 0.0)


# ---- at the inputs the GPU runs (PR.GPU_CASES, the list tests/test_gpu_markov_predict.py iterates): the restatement the device is
# judged against is tied to the dense definition THERE, the four controls must miss the GPU bound there, and what is fp32 on
# the device -- its inputs (the cases are fp32-exact) and the draw's output -- stays within half of the GPU bound.
GPU_WORST = {}


def teardown_module(module):
    for k, w in sorted(GPU_WORST.items()):
        print(f"GPU inputs: {k}: {w:.3e}")


@pytest.mark.parametrize("group", PR.GPU_GROUPS)
def test_gpu_inputs_restatement_controls_and_fp32_outputs(group):
    for c in (c for c in PR.GPU_CASES if c["group"] == group):
        x, xs, v, mu, m, rho, gamma = PR.case_inputs(c)
        t = PR.gpu_tol(c["N"])
        for b in c["series"]:
            pl = PR.plan(x, xs, v, mu[b], m[b], rho[b], gamma[b])
            # the fp32 evaluation: the recurrences are fp64 on the device too; fp32 is the output, rounded once
            eps = PR.case_eps(c, len(pl["steps"]))[b].astype(np.float64)
            for part in c["parts"]:
                r = PR.draw(pl, eps, part=part, exp=c["exp"])
                bound = t * max(1.0, np.abs(r).max()) + 2.0 ** -23 * np.abs(r)
                ratio = (np.abs(r.astype(np.float32).astype(np.float64) - r) / bound).max()
                GPU_WORST["fp32 output, largest error / GPU bound"] = max(GPU_WORST.get("fp32 output, largest error / GPU bound", 0.0), ratio)
                assert ratio <= 0.5, (c, b, part, ratio)
            if c["N"] > PR.DENSE_NMAX:
                # N = 2047 .. 8194: the dense definition needs N x N solves of seconds each (0.5 GB per matrix at 8194).  These
                # cases exist for the device scan's run / wave / chunk edges; the restatement's loops have no such edge
                continue
            dense = PR.dense_definition(x, xs, v, mu[b], m[b], rho[b], gamma[b])
            err = _errors(x, xs, v, mu[b], m[b], rho[b], gamma[b], dense=dense)
            assert err["cross"] == 0.0
            for k in ("mean", "var_q", "var_p", "chain", "bridge"):
                GPU_WORST["restatement vs dense, " + k] = max(GPU_WORST.get("restatement vs dense, " + k, 0.0), err[k])
                assert err[k] <= BOUND, (c, b, k, err[k])
            for variant in PR.VARIANTS:
                acts, quantity = PR.control_can_act(variant, x, xs)
                e = _errors(x, xs, v, mu[b], m[b], rho[b], gamma[b], variant=variant, dense=dense)
                if acts:
                    key = f"control {variant}, smallest miss / GPU bound"
                    GPU_WORST[key] = min(GPU_WORST.get(key, np.inf), e[quantity] / t)
                    assert e[quantity] > 10 * t, (c, b, variant, quantity, e[quantity])
                elif variant in ("no_cross", "anchor_zero"):           # ... and changes nothing elsewhere.  (Not asserted for the
                    # other two: beyond the grid the free increment still changes the DRAW's bridges, and Phi's sign the
                    # covariance BETWEEN points on different knots whenever the chain travels an odd number of steps)
                    assert max(e[k] for k in ("mean", "var_q", "var_p", "chain", "bridge")) <= BOUND, (c, b, variant, e)


def test_entry_points_validate_arguments_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    names = ("volt_markov_predict_workspace_bytes", "volt_markov_predict_plan_f32", "volt_markov_predict_draw_f32")
    for name in names:
        assert name in _lib.EXPORTS
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "volt_amd", "csrc", "libvolt_hip.so")],
                          capture_output=True, text=True).stdout
    for name in names:
        assert f" T {name}" in syms
    plan = L.volt_markov_predict_plan_f32
    # (x, xs, vol, jitter, mu, m, rho, gamma, mean, var_q, var_p, coef, code, steps, info, workspace, B, N, H, stream)
    order = ("x", "xs", "vol", "mu", "m", "rho", "gamma", "mean", "var_q", "var_p", "coef", "code", "steps", "info", "ws")

    def call(B=2, N=5, H=3, **kw):
        a = {k: 1 for k in order}
        a["ws"] = 256
        a.update(kw)
        p = [a[k] for k in order]
        return plan(*p[:3], 1e-3, *p[3:], B, N, H, None)
    for name, code in zip(order, (-1, -2, -3, -5, -6, -7, -8, -9, -10, -11, -12, -13, -14, -15, -16)):
        assert call(**{name: None}) == code, name
    assert call(ws=264) == -16                                         # not 256-byte aligned
    assert call(B=0) == -17 and call(B=65536) == -17 and call(N=0) == -18
    assert call(H=0) == -19 and call(H=2 ** 24 + 1) == -19
    draw = L.volt_markov_predict_draw_f32      # (mean, coef, code, steps, eps, out, B, S, H, E, flags, stream)
    for k in range(6):
        ptrs = [1] * 6
        ptrs[k] = None
        assert draw(*ptrs, 2, 3, 5, 16, 0, None) == -(k + 1)
    assert draw(*[1] * 6, 0, 3, 5, 16, 0, None) == -7 and draw(*[1] * 6, 65536, 3, 5, 16, 0, None) == -7
    assert draw(*[1] * 6, 2, 0, 5, 16, 0, None) == -8
    assert draw(*[1] * 6, 2, 3, 0, 16, 0, None) == -9
    assert draw(*[1] * 6, 2, 3, 5, 0, 0, None) == -10
    assert draw(*[1] * 6, 2, 3, 5, 16, 8, None) == -11
    assert (_lib.DRAW_EXP, _lib.PREDICT_NO_CHAIN, _lib.PREDICT_NO_BRIDGE) == (1, 2, 4)


def test_workspace_formula():
    from volt_amd import _lib
    L = _lib.lib()
    al = lambda b: (b + 255) // 256 * 256
    for B, N, H in ((1, 1, 1), (1, 399, 20), (3, 130, 300), (65, 399, 100), (2, 65536, 100)):
        # s, Phi and r in fp64 over the grid, the located interval of every test point: O(B (N + H))
        assert L.volt_markov_predict_workspace_bytes(B, N, H) == 3 * al(8 * B * N) + al(4 * B * H)
    assert L.volt_markov_predict_workspace_bytes(2, 65536, 100) <= 4 * 2 ** 20
    for bad in ((0, 5, 3), (65536, 5, 3), (2, 0, 3), (2, 5, 0), (2, 5, 2 ** 24 + 1)):
        assert L.volt_markov_predict_workspace_bytes(*bad) == 0


def test_python_validation_and_unchanged_refusals():
    from volt_amd import gp, ops
    from volt_amd._lib import VoltHipError
    from volt_amd.kernels import BMKernel
    from volt_amd.models import SingleTaskVariationalGP
    from volt_amd.variational import MarkovVariationalLatent, _predict_points
    x = torch.arange(1., 9.) / 252
    build = lambda solver: SingleTaskVariationalGP(init_points=x.view(-1, 1), covar_module=BMKernel(), mean_module=gp.ConstantMean(),
                                                   learn_inducing_locations=False, use_whitened_var_strat=False, prior_solver=solver)
    other = x[:3] + 0.001
    for solver in ("dense", "linear"):                                 # word for word what they raised before
        with pytest.raises(NotImplementedError, match=re.escape(
                "SingleTaskVariationalGP(x) away from the inducing points is outside the accelerated path: LearnGPCV only "
                "evaluates the model at train_x (train_utils.py:51,60)")):
            build(solver)(other)
    model = build("markov")
    assert isinstance(model(x), MarkovVariationalLatent) and isinstance(model(x.view(-1, 1)), MarkovVariationalLatent)
    for bad in (torch.zeros(2, 2), torch.zeros(0), torch.tensor([0.1, -0.1]), torch.tensor([float("nan")]),
                torch.tensor([float("inf")]), torch.zeros(2, 1, 1)):
        with pytest.raises(ValueError, match="test points"):
            model(bad)
    with pytest.raises(VoltHipError):                                  # a valid request on the CPU: no fallback
        model(other)
    assert _predict_points(torch.tensor([[0.3], [0.1]]), "t").tolist() == pytest.approx([0.3, 0.1])
    a = torch.zeros(1, 8)
    with pytest.raises(VoltHipError):
        ops.markov_predict_plan(x, other, torch.tensor([0.2]), torch.tensor([0.0]), a, a, a)


def test_predict_kernels_cross_compile_without_scratch_or_spills(tmp_path):
    from volt_amd.build import FLAGS, SOURCES, _hipcc
    assert "markov_predict.hip" in SOURCES
    src = os.path.join(ROOT, "volt_amd", "csrc", "markov_predict.hip")
    r = subprocess.run([_hipcc(), *FLAGS, "-c", src, "-o", str(tmp_path / "markov_predict.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel, count in (("markov_predict_plan_kernel", 1), ("markov_predict_draw_kernel", 4)):
        blocks = [b for b in r.stderr.split("Function Name: ")[1:] if kernel in b.split()[0]]
        assert len(blocks) == count, [b.split()[0] for b in blocks]    # the draw: 16-byte or single accesses of eps and of out
        for b in blocks:
            name = b.split()[0]
            assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, name
            assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, name
            print(name, "VGPRs", re.search(r" VGPRs: (\d+)", b).group(1), "occupancy",
                  re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1), "static LDS",
                  re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    with open(src) as fh:
        text = fh.read()
    assert "atomic" not in text.replace("no atomics", "")
    for pinned in ("gpcv_markov_step_kernel", "markov_root_draw_kernel", "markov_root_var_kernel"):
        assert pinned not in text                                      # tests/test_gpcv_markov_host.py counts those by name


@pytest.mark.parametrize("T", [1, 3, 8])
def test_multitask_composition_matches_the_dense_kronecker_definition(T):
    worst = {"mean": 0.0, "var": 0.0, "cov": 0.0}
    for N in (1, 2, 17, 65):
        for x0, v, regime in ((0.0, 0.2, "random"), (PR.DT, 0.9, "startup"), (PR.DT, 0.05, "weak")):
            x = PR.make_grid(N, x0)
            _, rho, gamma, _ = PR.make_params(x, v, regime)
            M = PR.f32(np.random.default_rng(N + T).normal(-1.0, 0.5, (N, T)))
            Lt, f, raw_var, c = PR.make_task_params(T)
            xs = PR.make_points(x, "mixed")
            mean_d, C = PR.mt_dense_definition(x, xs, v, c, M, rho[0], gamma[0], Lt, f, raw_var)
            mean, var, Gk, Gb = PR.mt_maps(x, xs, v, c, M, rho[0], gamma[0], Lt, f, raw_var)
            sc = np.abs(C).max()
            worst["mean"] = max(worst["mean"], np.abs(mean - mean_d).max() / max(1.0, np.abs(mean_d).max()))
            worst["var"] = max(worst["var"], np.abs(var.reshape(-1) - np.diag(C)).max() / sc)
            worst["cov"] = max(worst["cov"], np.abs(Gk @ Gk.T + Gb @ Gb.T - C).max() / sc)
            assert np.abs(Gk @ Gb.T).max() == 0.0
    print(f"multi-task, T = {T}: largest error / scale", {k: f"{w:.2e}" for k, w in worst.items()})
    assert max(worst.values()) <= BOUND, worst


def test_multitask_refusals_and_validation():
    from volt_amd.kernels import BMKernel
    from volt_amd.models import MultitaskVariationalGP
    x = torch.arange(1., 9.) / 252
    with pytest.raises(NotImplementedError, match="away from the inducing points"):      # "dense" keeps raising
        MultitaskVariationalGP(x, num_tasks=2, covar_module=BMKernel())(x[:3] + 0.001)
    model = MultitaskVariationalGP(x, num_tasks=2, covar_module=BMKernel(), prior_solver="markov")
    for bad in (torch.zeros(2, 2), torch.tensor([0.1, -0.1]), torch.tensor([float("nan")])):
        with pytest.raises(ValueError, match="test points"):
            model(bad)
