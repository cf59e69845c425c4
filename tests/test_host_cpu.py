"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/volt_hip.h
declares, argument validation is reachable without a device, host logic (sharding, synthetic data,
parameter order) behaves, and the product path refuses to run without the GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from volt_amd import _lib
    from volt_amd.build import build_lib
    build_lib()                                             # hipcc cross-compiles gfx950 without a GPU
    handle = _lib.lib()
    for hname, table, least in (("volt_hip.h", _lib.EXPORTS, 15), ("volt_hip_tune.h", _lib.TUNE_EXPORTS, 4)):
        header = open(os.path.join(ROOT, "include", hname)).read()
        declared = sorted(set(re.findall(r"\b(volt_[a-z0-9_]+)\s*\(", header)))
        assert len(declared) >= least
        for name in declared:
            assert hasattr(handle, name), f"{name} declared in {hname} but not exported"
            assert name in table, f"{name} has no ctypes signature in volt_amd/_lib.py"
        assert sorted(table) == declared, (hname, sorted(set(table) ^ set(declared)))
    # the product boundary carries no measurement / tuning entry points
    assert not [n for n in _lib.EXPORTS if "tune" in n or "profile" in n or "describe" in n]
    assert handle.volt_abi_version() == _lib.ABI_VERSION
    assert handle.volt_padded_n(1) == 128 and handle.volt_padded_n(4096) == 4096 and handle.volt_padded_n(4097) == 4224


def test_argument_validation_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    assert L.volt_fill_f32(None, None, 1, 8, 8, 64, None) == -1
    assert L.volt_cumtrapz_f32(1, 8, 1, 0, 1, 1, 1, 1, None) == -7            # N < 2: x[1]-x[0] undefined
    assert L.volt_potrf_f32(1, 1, 1, 1, 100, None) == -5                      # Np not a multiple of 128
    assert L.volt_potrf_ws_f32(1, 1, 1, 1, 100, None, 0, 0, None) == -5
    assert L.volt_potrf_k_f32(None, 8, 64, None, 0.0, 1, 1, 1, 1, 8, None, 0, 0, None) == -1
    assert L.volt_potrf_k_f32(1, 4, 64, None, 0.0, 1, 1, 1, 1, 8, None, 0, 0, None) == -2     # row stride shorter than N
    assert L.volt_potrf_workspace_bytes(1, 100) == 0
    assert L.volt_potrf_workspace_bytes(1, 128) == 0 and L.volt_potrf_workspace_bytes(4, 256) == 0   # nothing long enough to cut
    tables = ((33 * 8 * (1 + 4 * 33) + 16) * 16 + 255) // 256 * 256  # the balanced schedule's tables (+ a 16-slot header) live in caller scratch too
    # round 5: + the one-launch factorisation's piece list (16 B per piece, 16-slot header) and progress words (3 n ints per matrix)
    pieces = lambda B, n: B * sum(1 + (1 if 1 <= k <= n - 2 else 0) + (n - k - 1) for k in range(n))
    al = lambda b: (b + 255) // 256 * 256
    # round 6: + the queue words of the pullers (8 queues x 32 ints: head and claim of each on a line of its own)
    batch = lambda B, n: al((16 + pieces(B, n)) * 16) + al((B * ((3 * n + 31) // 32 * 32) + 8 * 32) * 4)
    assert L.volt_potrf_workspace_bytes(8, 4096) == 64 * 33 * 65536 + (33 * 33 * 8 * 4 + 255) // 256 * 256 + tables + batch(8, 32)
    assert L.volt_potrf_workspace_bytes(65, 4096) == batch(65, 32)        # above 64 matrices: no slabs, the piece list alone
    assert L.volt_batch_describe(8, 32, 0, 0, None, 0) == pieces(8, 32)
    assert L.volt_potrf_workspace_bytes(64, 4096) > 128 * 33 * 65536
    # the fp64 twins (round 5: the one-launch schedule's progress words; csrc/batch64_step.hip)
    assert L.volt_potrf_ws_f64(1, 1, 1, 1, 100, None, 0, None) == -5
    assert L.volt_potrf_ws_f64(1, 1, 1, 1, 128, 3, 4096, None) == -6                  # scratch not 256-byte aligned
    assert L.volt_potrf_k_f64(None, 8, 64, None, 0.0, 1, 1, 1, 1, 8, None, 0, None) == -1
    assert L.volt_potrf_k_f64(1, 4, 64, None, 0.0, 1, 1, 1, 1, 8, None, 0, None) == -2    # row stride shorter than N
    assert L.volt_potrf_k_f64(1, 8, 64, None, 0.0, None, 1, 1, 1, 8, None, 0, None) == -6
    assert L.volt_potrf_workspace_bytes_f64(1, 100) == 0 and L.volt_potrf_workspace_bytes_f64(1, 128) == 0   # one block column: nothing to hand on
    words = lambda B, n: ((B * ((5 * n + 1 + 31) // 32 * 32) + 8 * 32) * 4 + 255) // 256 * 256   # progress words + the pullers' queue words (round 6)
    assert L.volt_potrf_workspace_bytes_f64(1, 4096) == words(1, 32) and L.volt_potrf_workspace_bytes_f64(8, 1024) == words(8, 8)
    assert L.volt_potrf_workspace_bytes_f64(512, 4096) == 0                           # beyond the measured range: launch per block column
    assert (L.volt_mll_workspace_bytes_f64(8, 4096, 1) - L.volt_mll_workspace_bytes_f64(8, 4096, 0)
            >= 8 * 4096 * 4096 * 8 + 8 * 528 * 8)                                    # + Y, one norm partial per tile
    assert L.volt_mll_workspace_bytes(64, 4096, 1) > L.volt_mll_workspace_bytes(64, 4096, 0) > 0
    # the one-launch step for short series keeps its state and alpha's partial sums in the workspace: there for
    # the shapes it takes (few series of N <= 1024, gradient step), absent where the library keeps the launch-per-column path
    base = lambda B, N: L.volt_mll_workspace_bytes(B, N, 1) / B
    assert base(32, 399) > base(64, 399) and base(64, 256) > base(128, 256)
    assert L.volt_mll_workspace_bytes(8, 399, 1) - L.volt_mll_workspace_bytes(8, 399, 0) > 8 * 512 * 512 * 4   # + Y, partials, state
    assert L.volt_rollout_scratch_bytes(2, 3, 4) == 2 * 3 * 16 * 4
    assert L.volt_mll_workspace_init_f32(None, 8, 4096, 1, None) == -1 and L.volt_potrf_workspace_init_f32(None, 0, 8, 100, None) == -4
    assert L.volt_potrf_workspace_init_f32(None, 0, 100, 256, None) == 0           # no scratch for that shape: nothing to do
    assert L.volt_potrf_workspace_init_f32(None, 0, 100, 4096, None) == -1         # (100 matrices of N = 4096 have the piece list)
    with pytest.raises(_lib.VoltHipError):
        _lib.check(-3, "x")


def test_product_path_has_no_cpu_fallback():
    from volt_amd import ops
    from volt_amd._lib import VoltHipError
    with pytest.raises(VoltHipError):
        ops.fill(torch.zeros(8))
    with pytest.raises(VoltHipError):
        ops.cumtrapz(torch.ones(8), torch.arange(8.))
    from volt_amd.kernels import VolatilityKernel
    with pytest.raises(VoltHipError):
        VolatilityKernel().forward(torch.arange(8.).unsqueeze(-1), torch.ones(8, 1))


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "volt_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("oracle/", "").lower() or f == "synthetic.py" or \
                    "import oracle" not in src and "from oracle" not in src, f
                assert "from oracle" not in src and "import oracle" not in src, f"{f} imports the oracle"


def test_shard_range_partitions_contiguously():
    from volt_amd.distributed import shard_range
    for total, world in ((256, 8), (64, 8), (10, 4), (3, 8)):
        spans = [shard_range(total, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1


def test_synthetic_series_are_reproducible_and_rank_shardable():
    from volt_amd.synthetic import sde_batch, sde_series
    x, F, V = sde_batch(4, 64, seed=2019)
    _, F2, V2 = sde_batch(2, 64, seed=2019, first=2)
    assert np.array_equal(F[2:], F2) and np.array_equal(V[2:], V2)
    f, v = sde_series(64, 2019)
    assert np.array_equal(f, F[0]) and (F > 0).all() and (V >= 1e-3).all()
    assert x.dtype == np.float32 and abs(x[1] - 1 / 252.) < 1e-9


def test_parameter_order_matches_positional_grad_flags():
    """train_utils.py:226-227 freezes parameters by POSITION: the likelihood noise must come first, then
    the mean parameters, then the vol model's."""
    from volt_amd import gp
    from volt_amd.means import LogLinearMean

    class M(gp.ExactGP):
        def __init__(self):
            super().__init__(torch.arange(4.), torch.zeros(4), gp.GaussianLikelihood())
            self.mean_module = gp.ConstantMean()
            self.vol_lh = gp.GaussianLikelihood()
    m = M()
    names = [n for n, _ in m.named_parameters()]
    assert names[0] == "likelihood.noise_covar.raw_noise" and names[1] == "mean_module.constant"
    m.mean_module = LogLinearMean(1)
    names = [n for n, _ in m.named_parameters()]
    assert names[:3] == ["likelihood.noise_covar.raw_noise", "mean_module.weights", "mean_module.bias"]
    lh = gp.GaussianLikelihood()
    lh.raw_noise.data = torch.tensor([1e-5])
    assert abs(float(lh.noise) - 0.6932522) < 1e-6
    lh.noise = 0.25
    assert abs(float(lh.noise) - 0.25) < 1e-6
    assert m.train_inputs[0].shape == (4, 1)                     # 1-D inputs stored as [N,1] like gpytorch


def test_install_as_voltron_alias():
    import importlib
    import sys
    import volt_amd
    saved = {k: v for k, v in sys.modules.items() if k == "voltron" or k.startswith("voltron.")}
    try:
        volt_amd.install_as_voltron()
        assert importlib.import_module("voltron.kernels").VolatilityKernel is volt_amd.VolatilityKernel
        assert importlib.import_module("voltron.rollout_utils").Rollouts is volt_amd.Rollouts
    finally:
        for k in [k for k in sys.modules if k == "voltron" or k.startswith("voltron.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_gpcv_stage_refuses_cpu_tensors_and_validates_arguments():
    """LearnGPCV has no CPU path either; its C entry validates before touching the device."""
    from volt_amd import _lib
    from volt_amd.train_utils import LearnGPCV
    L = _lib.lib()
    assert L.volt_gpcv_workspace_bytes(2, 300, 1) > L.volt_gpcv_workspace_bytes(2, 300, 0) > L.volt_mll_workspace_bytes(2, 300, 1)
    assert L.volt_gpcv_step_f32(None, 8, 64, 1e-3, *([None] * 6), 75, 1e-6, 1e-3, 1.0, 1.0, *([None] * 7), 1, 8, 0, None) == -1
    assert L.volt_gemm_nt_f32(256, 128, 0, 0, 256, 128, 0, 0, 256, 128, 0, 0, 1.0, 0.0, 1, 100, 128, 128, None) == -16
    assert L.volt_mll_grad_k_f32(None, None, None, None, 1, 8, None) == -1
    assert L.volt_rollout_shared_f32(*([None] * 8), 1, 1, 4, 5, 0, 0.5, None) == -1
    x = torch.arange(50, dtype=torch.float32) / 252
    with pytest.raises(_lib.VoltHipError):
        LearnGPCV(x, torch.rand(51) + 1.0, train_iters=1)

    # volt_gemm_nt_f32: every return code of csrc/gpcv.hip, none of which reaches a launch (the pointers are small integers).
    # A code is minus the position of the argument it blames; bsc (11), alpha (13) and beta (14) have no condition to fail.
    def gemm(**kw):
        a = dict(A=256, lda=128, bsa=0, uplo_a=0, B=256, ldb=128, bsb=0, uplo_b=0, C=256, ldc=128, bsc=0, uplo_c=0,
                 alpha=1.0, beta=0.0, batch=1, M=128, N=128, K=128, stream=None)
        assert not set(kw) - set(a)
        a.update(kw)
        return L.volt_gemm_nt_f32(*a.values())
    for code, cases in ((-1, [dict(A=None)]),
                        (-2, [dict(lda=127), dict(K=256, lda=128), dict(lda=130), dict(A=260)]),   # < K, % 4, misaligned A
                        (-3, [dict(bsa=2)]),
                        (-4, [dict(uplo_a=3), dict(uplo_a=-1)]),
                        (-5, [dict(B=None)]),
                        (-6, [dict(ldb=124), dict(ldb=129), dict(B=264)]),
                        (-7, [dict(bsb=6)]),
                        (-8, [dict(uplo_b=3), dict(uplo_b=-1)]),
                        (-9, [dict(C=None)]),
                        (-10, [dict(ldc=127), dict(N=256, ldc=255)]),
                        (-12, [dict(uplo_c=3), dict(uplo_c=-1)]),
                        (-15, [dict(batch=-1)]),
                        (-16, [dict(M=0), dict(M=100), dict(M=-128)]),
                        (-17, [dict(N=0), dict(N=130, ldc=130)]),
                        (-18, [dict(K=0), dict(K=64), dict(K=132, lda=132, ldb=132)])):
        for kw in cases:
            assert gemm(**kw) == code, (code, kw)
    assert gemm(batch=0) == 0                                   # nothing to do: no launch
    assert gemm(batch=0, lda=127) == -2                         # ... but validated all the same

    # volt_ewma_f32(y, bs_y, w, k, out, B, N, stream)
    def ewma(**kw):
        a = dict(y=256, bs_y=8, w=256, k=5, out=256, B=1, N=8, stream=None)
        assert not set(kw) - set(a)
        a.update(kw)
        return L.volt_ewma_f32(*a.values())
    for code, cases in ((-1, [dict(y=None)]), (-3, [dict(w=None)]), (-4, [dict(k=0), dict(k=16385), dict(k=-1)]),
                        (-5, [dict(out=None)]), (-6, [dict(B=65536), dict(B=-1)]), (-7, [dict(N=0)])):
        for kw in cases:
            assert ewma(**kw) == code, (code, kw)
    assert ewma(B=0) == 0 and ewma(B=0, k=16384) == 0
    assert ewma(B=0, N=0) == -7

    # volt_adam_step_f32(slots, nslots, total, grad, lr, beta1, beta2, eps, state, stream)
    def adam(**kw):
        a = dict(slots=256, nslots=1, total=1, grad=256, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, state=256, stream=None)
        assert not set(kw) - set(a)
        a.update(kw)
        return L.volt_adam_step_f32(*a.values())
    for code, cases in ((-1, [dict(slots=None)]), (-2, [dict(nslots=0), dict(nslots=-1)]), (-3, [dict(total=0), dict(total=-5)]),
                        (-4, [dict(grad=None)]), (-9, [dict(state=None)])):
        for kw in cases:
            assert adam(**kw) == code, (code, kw)


def test_reference_call_sites_resolve_through_the_aliases():
    """example.ipynb cells 0 and 8 and train_utils.py reach everything by name: voltron.* and gpytorch.*."""
    import importlib
    import sys
    import volt_amd
    had = {k: sys.modules.get(k) for k in list(sys.modules) if k == "gpytorch" or k.startswith("gpytorch.")}
    try:
        volt_amd.install_as_voltron()
        import gpytorch
        from voltron.likelihoods import VolatilityGaussianLikelihood
        from voltron.models import SingleTaskVariationalGP, VoltronGP, VoltMagpie, BMGP      # noqa: F401
        from voltron.kernels import BMKernel, VolatilityKernel, FBMKernel                                  # noqa: F401
        from voltron.train_utils import TrainVolModel, TrainVoltMagpieModel, LearnGPCV, TrainDataModel  # noqa: F401
        from voltron.rollout_utils import Rollouts, GeneratePrediction, nonvol_rollouts                     # noqa: F401
        x = torch.arange(12.) / 252
        lik = VolatilityGaussianLikelihood(param="exp")
        model = SingleTaskVariationalGP(init_points=x.view(-1, 1), likelihood=lik, use_piv_chol_init=False,
                                        mean_module=gpytorch.means.ConstantMean(), covar_module=BMKernel(),
                                        learn_inducing_locations=False, use_whitened_var_strat=False)
        mll = gpytorch.mlls.VariationalELBO(lik, model, 12, combine_terms=True)
        with gpytorch.settings.num_gauss_hermite_locs(75):
            from volt_amd.variational import num_gauss_hermite_locs
            assert num_gauss_hermite_locs.value() == 75
        assert num_gauss_hermite_locs.value() == 20
        assert [n for n, _ in model.named_parameters()][:2] == [
            "variational_strategy._variational_distribution.variational_mean",
            "variational_strategy._variational_distribution.chol_variational_covar"]
        with gpytorch.settings.max_cholesky_size(2000):                     # GPGenerator.py:62
            pass
        importlib.import_module("gpytorch.utils.cholesky").psd_safe_cholesky
        assert isinstance(mll, gpytorch.mlls.VariationalELBO)
    finally:
        for k in [k for k in sys.modules if k == "gpytorch" or k.startswith("gpytorch.")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in had.items() if v is not None})


def _reference_surface():
    """The reference's public surface as recorded names (tests/golden/make_reference_surface.py parses its files)."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_surface.json")) as fh:
        return json.load(fh)


def test_reference_train_utils_imports_against_our_namespaces():
    """The reference's own voltron/train_utils.py and rollout_utils.py import cleanly when ``voltron`` and ``gpytorch``
    resolve to this package: every ``gpytorch.<sub>.<attr>`` they look up (recorded in tests/golden/reference_surface.json)
    exists here with the reference's spelling."""
    import sys
    import volt_amd
    surface = _reference_surface()["gpytorch_attrs"]
    assert sorted(surface) == ["rollout_utils.py", "train_utils.py"] and surface["train_utils.py"]
    had = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in ("gpytorch", "voltron")}
    try:
        volt_amd.install_as_voltron()
        for rel, names in sorted(surface.items()):
            import gpytorch
            for sub, attr in names:
                assert hasattr(getattr(gpytorch, sub), attr), f"gpytorch.{sub}.{attr} used by {rel} is missing"
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in ("gpytorch", "voltron")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in had.items() if v is not None})


def test_public_signatures_match_the_reference():
    """Same function names, argument names, order and defaults as voltron/train_utils.py and rollout_utils.py
    (keyword-only extras such as ``z=`` / ``pred_vol=`` are additions)."""
    import inspect
    from volt_amd import rollout_utils, train_utils
    surface = _reference_surface()["functions"]
    for mod, rel in ((train_utils, "train_utils.py"), (rollout_utils, "rollout_utils.py")):
        assert surface[rel], rel
        for name, ref in surface[rel].items():
            names, defaults = ref["args"], ref["defaults"]
            if name == "TrainBasicModel":                  # out of scope (lives in baselines/, not the product)
                continue
            assert hasattr(mod, name), f"{rel}:{name} has no counterpart"
            sig = inspect.signature(getattr(mod, name))
            pos = [p for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
            assert [p.name for p in pos][:len(names)] == names, (name, [p.name for p in pos], names)
            ours = [p.default for p in pos[:len(names)] if p.default is not inspect.Parameter.empty]
            assert ours == defaults, (name, ours, defaults)


def test_class_surfaces_match_the_reference():
    """Every class of the reference's path files exists here under the same module path, with the same constructor
    argument names / order and at least the same public methods ("same names, argument order, defaults")."""
    import importlib
    import inspect
    files = {"models/VoltMagpie.py": ["VoltMagpie"], "models/VoltronGP.py": ["VoltronGP"], "models/Volt.py": ["Volt"],
             "models/BMGP.py": ["BMGP"],
             "models/single_task_variational_gp.py": ["SingleTaskVariationalGP"],
             "means/EWMA.py": ["EWMAMean", "DEWMAMean", "TEWMAMean", "MeanRevertingEMAMean"],
             "means/loglinear_mean.py": ["LogLinearMean"], "kernels/VolKernel.py": ["VolatilityKernel"],
             "kernels/BMKernel.py": ["BMKernel"], "kernels/FBMKernel.py": ["FBMKernel"],
             "likelihoods/volatility_likelihood.py": ["VolatilityGaussianLikelihood"]}
    surface = _reference_surface()["classes"]
    for rel, classes in files.items():
        assert sorted(surface[rel]) == sorted(classes), (rel, sorted(surface[rel]))
        ours = importlib.import_module("volt_amd." + rel[:-3].replace("/", "."))
        for cname, ref in surface[rel].items():
            cls = getattr(ours, cname)
            for fn in ref["methods"]:
                assert hasattr(cls, fn), f"{rel}:{cname}.{fn} missing"
            if ref["init_args"] is not None:
                want = ref["init_args"]
                got = [p.name for p in inspect.signature(cls.__init__).parameters.values()
                       if p.kind == p.POSITIONAL_OR_KEYWORD][1:]
                assert got[:len(want)] == want, (rel, cname, got, want)


def test_bench_refuses_gpus_it_cannot_see():
    """`python bench.py --gpus N` on a box with fewer than N GPUs (here: none) exits non-zero with a clear message and
    prints NO JSON line -- it never reports an N-GPU figure from fewer ranks."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "VOLT_BENCH_ONE_DEVICE")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has the GPUs")
    assert out.returncode == 2
    assert "needs 2 visible GPUs" in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]


def test_deferred_checks_keep_one_accumulator_per_shape():
    """gp.deferred_checks: factorisations of different batch shapes inside one iteration (an MLL step and a GPCV step,
    two models) keep their failure flags apart; nothing is dropped when the shape changes."""
    from volt_amd import gp
    with gp.deferred_checks() as chk:
        assert gp.deferred_checks.deferring() is chk
        chk.note(torch.tensor([0, 3, 0], dtype=torch.int32))
        chk.note(torch.tensor([0], dtype=torch.int32))                    # another shape: the first accumulator stays
        chk.note(torch.tensor([0, 0, 0], dtype=torch.int32))
        assert chk.any_bad() == 1
        chk.note(torch.tensor([5], dtype=torch.int32))
        assert chk.any_bad() == 2
        with pytest.raises(gp.NotPSDError):
            chk.raise_if_bad()
        chk.clear()
        assert chk.any_bad() == 0
        chk.immediate = True
        assert gp.deferred_checks.deferring() is None and gp.deferred_checks._active is chk
    assert gp.deferred_checks._active is None


def test_graph_capture_is_the_default_where_a_step_is_launch_bound():
    """graph=None (what every reference call site passes: nothing, voltron/train_utils.py:15,69,98,192) captures the
    iteration where its estimated GPU time is below CAPTURE_BELOW_MS; an explicit True / False is honoured; never on a CPU
    tensor (there is no CPU path to capture)."""
    import torch
    from volt_amd.train_utils import _auto_graph, _capture_pays
    assert _capture_pays(torch.empty(1, 4096)) and _capture_pays(torch.empty(4096)) and _capture_pays(torch.empty(64, 399))
    assert _capture_pays(torch.empty(399)) and _capture_pays(torch.empty(64, 2048))
    assert not _capture_pays(torch.empty(64, 4096)) and not _capture_pays(torch.empty(16, 4096))
    # the GPCV ELBO step is 5 N^3 / 3, not 2 N^3 / 3: its gate has its own cost model
    assert _capture_pays(torch.empty(32, 2048)) and not _capture_pays(torch.empty(32, 2048), n3_coeff=5.0 / 3.0)
    assert _auto_graph(True, torch.empty(64, 4096)) is True and _auto_graph(False, torch.empty(399)) is False
    assert _auto_graph(None, torch.empty(399)) is False              # a CPU tensor: nothing to capture


def test_reference_driver_imports_resolve():
    """ADVICE r3 / INTEGRATION 2: after install_as_voltron() every `from voltron... import` / `from gpytorch... import`
    name of the reference's drivers resolves -- including the out-of-scope baselines they import unconditionally
    (TrainBasicModel, MaternGP / SMGP, gpytorch.kernels.*), which come lazily from baselines/ or as call-time stand-ins."""
    import importlib
    import volt_amd
    volt_amd.install_as_voltron()
    wanted = {
        "voltron.train_utils": ["LearnGPCV", "TrainVolModel", "TrainVoltMagpieModel", "TrainBasicModel", "TrainDataModel"],
        "voltron.models": ["VoltMagpie", "VoltronGP", "BMGP", "MaternGP", "SMGP", "SingleTaskVariationalGP"],
        "voltron.means": ["EWMAMean", "DEWMAMean", "TEWMAMean", "LogLinearMean"],
        "voltron.rollout_utils": ["GeneratePrediction", "Rollouts", "nonvol_rollouts"],
        "voltron.kernels": ["VolatilityKernel", "BMKernel", "FBMKernel"],
        "gpytorch.kernels": ["SpectralMixtureKernel", "MaternKernel", "RBFKernel", "ScaleKernel"],
        "gpytorch.likelihoods": ["GaussianLikelihood"], "gpytorch.mlls": ["ExactMarginalLogLikelihood"],
        "gpytorch.means": ["ConstantMean", "LinearMean"],
    }
    # ... and whatever the drivers really import from those packages (stocks/GenerateMultiMeanPreds.py, weather/GPGenerator.py,
    # weather/BasicWind.py; voltron.data's network download helpers are out of scope)
    drivers = _reference_surface()["driver_imports"]
    assert drivers
    for mod, names in drivers.items():
        wanted.setdefault(mod, [])
        wanted[mod] += names
    for mod, names in wanted.items():
        m = importlib.import_module(mod)
        for name in names:
            assert getattr(m, name) is not None, (mod, name)
    # a stand-in raises when CALLED, with a pointer to baselines/ -- never at import
    from volt_amd import _out_of_scope
    with pytest.raises(NotImplementedError, match="baselines/"):
        _out_of_scope._stand_in("TrainBasicModel")(None, None)
    with pytest.raises(NotImplementedError):
        _out_of_scope._stand_in("MaternGP")(None)


def test_fp64_device_assembly_dpp_hazards_and_kernel_shape():
    """Round 6 (csrc/tiles64.h): the fp64 pivot phase and sub-block inverse use v_fmac_f64_dpp row_newbcast from inline asm, where
    the compiler's hazard recogniser cannot see the DPP operand -- every such instruction in the cross-compiled assembly must have
    its operand's last VALU write >= 2 and any EXEC write >= 5 wait states ahead; and the one-launch kernel must keep the shape its
    speed depends on (<= 420 registers, the steady K loop one basic block of 128 MFMAs: DESIGN 4.7).  hipcc only, no GPU."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("check_dpp_hazards", os.path.join(os.path.dirname(__file__), "..", "scripts", "check_dpp_hazards.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for src in ("chol64.hip", "batch64_step.hip"):
        bad, n, text = m.check(src)
        assert n > 1000 and bad == 0, (src, n, bad)
    shapes = m.kernel_shape(text, "_ZN4volt19batch64_step_kernel")
    assert len(shapes) == 2
    for name, (regs, mfma) in shapes.items():
        assert regs <= 420 and mfma == 128, (name, regs, mfma)


def test_rollout_entries_argument_codes():
    """Every return code of csrc/rollout.hip's two entries.  A code is minus the position of the argument it blames; none of
    these calls reaches a launch (each has one fault, or G = 0 / S = 0: the pointers are small integers)."""
    from volt_amd import _lib
    L = _lib.lib()

    def bordered(**kw):
        a = dict(rho=256, tau=256, acc0=256, dx=256, hist_y=256, hist_e1=None, hist_e2=None, ema_prev=None, mr_latent=None,
                 latent=None, w=256, pred_vol=256, z=256, samples=256, scratch=None, info=256, G=0, S=3, H=8, k=5, mean_mode=0,
                 use_theta=0, theta=0.0, mr_theta=0.5, jitter=1e-4, stream=None)
        assert not set(kw) - set(a)
        a.update(kw)
        return L.volt_rollout_bordered_f32(*a.values())
    for code, cases in ((-1, [dict(rho=None)]), (-2, [dict(tau=None)]), (-3, [dict(acc0=None)]), (-4, [dict(dx=None)]),
                        (-5, [dict(hist_y=None)]),
                        (-6, [dict(mean_mode=1), dict(mean_mode=2, hist_e2=256), dict(mean_mode=4)]),     # hist_e1 missing
                        (-7, [dict(mean_mode=2, hist_e1=256)]),
                        (-8, [dict(mean_mode=3), dict(mean_mode=3, ema_prev=256), dict(mean_mode=3, mr_latent=256)]),
                        (-10, [dict(use_theta=1)]),
                        (-11, [dict(w=None)]), (-12, [dict(pred_vol=None)]), (-13, [dict(z=None)]), (-14, [dict(samples=None)]),
                        (-16, [dict(info=None)]), (-17, [dict(G=-1)]), (-18, [dict(S=-1)]),
                        (-19, [dict(H=0), dict(H=1025), dict(H=-1)]), (-20, [dict(k=0), dict(k=2049)]),
                        (-21, [dict(mean_mode=-1), dict(mean_mode=5)])):
        for kw in cases:
            assert bordered(**kw) == code, (code, kw)
    # nothing to do: no launch -- scratch (15) is optional, and the LDS refusal behind these checks cannot be reached from
    # H <= 1024, k <= 2048 (12 (k + H) + k floats is 152 KB there)
    assert bordered() == 0 and bordered(G=2, S=0) == 0 and bordered(H=1024, k=2048) == 0
    assert bordered(mean_mode=3, ema_prev=256, mr_latent=256) == 0 and bordered(use_theta=1, latent=256) == 0
    assert bordered(S=0, G=2, H=0) == -19                       # ... but validated all the same

    def shared(**kw):
        a = dict(hist_y=256, hist_e1=None, hist_e2=None, ema_prev=None, mr_latent=None, w=256, e=256, samples=256, G=0, S=3,
                 H=8, k=5, mean_mode=0, mr_theta=0.5, stream=None)
        assert not set(kw) - set(a)
        a.update(kw)
        return L.volt_rollout_shared_f32(*a.values())
    for code, cases in ((-1, [dict(hist_y=None)]), (-2, [dict(mean_mode=1), dict(mean_mode=2, hist_e2=256)]),
                        (-3, [dict(mean_mode=2, hist_e1=256)]),
                        (-4, [dict(mean_mode=3), dict(mean_mode=3, ema_prev=256), dict(mean_mode=3, mr_latent=256)]),
                        (-6, [dict(w=None)]), (-7, [dict(e=None)]), (-8, [dict(samples=None)]), (-9, [dict(G=-1)]),
                        (-10, [dict(S=-1)]), (-11, [dict(H=0), dict(H=4097)]), (-12, [dict(k=0), dict(k=2049)]),
                        (-13, [dict(mean_mode=-1), dict(mean_mode=4)]),
                        # the LDS refusal, 12 (k + H) + k floats > 160 KB, reported against H (it sits behind the G = 0 /
                        # S = 0 return, so it needs work to refuse: the smallest H refused at these k; nothing is launched)
                        (-11, [dict(G=1, k=2048, H=1195), dict(G=1, k=1, H=3413)])):
        for kw in cases:
            assert shared(**kw) == code, (code, kw)
    assert shared() == 0 and shared(G=2, S=0) == 0 and shared(G=0, k=2048, H=4096) == 0
