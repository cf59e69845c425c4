"""CPU-side checks of the path-summary stage (no GPU): the fp64 yardstick tests/scoring_ref.py against the reference's own
Pricer / ECDF results (tests/golden/scoring.npz, recorded by make_golden_scoring.py) and against the O(S^2) CRPS, the
argument validation and scratch size of volt_path_summary_f32, and the Python surface's behaviour without a device."""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scoring_ref  # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("scoring")


@pytest.fixture(scope="module")
def ref_on_fixture(fixture):
    """scoring_ref on the fixture's LOG prices with exp: [E expiries as series, S, 1 step], every expiry with the strikes."""
    log_p = torch.from_numpy(fixture["log_p"])                    # [S, E]
    E = log_p.shape[1]
    strikes = torch.from_numpy(fixture["strikes"]).reshape(1, -1).expand(E, -1)
    truth = torch.from_numpy(fixture["true_pxs"]).reshape(E, 1)
    return scoring_ref.summarize(log_p.t().unsqueeze(-1), truth=truth, strikes=strikes, exp=True)


def test_ref_reproduces_the_reference_percentiles_as_counts(fixture, ref_on_fixture):
    S, E = fixture["log_p"].shape
    M = fixture["strikes"].size
    n_lt = ref_on_fixture["counts"][:, 1, 0]
    pct = fixture["pct"].reshape(E, M)
    for e in range(E):
        assert 0 < int(n_lt[e]) < S
        for m in range(M):
            assert round(float(pct[e, m]) * S) == int(n_lt[e]), (e, m, pct[e, m], int(n_lt[e]))
        assert round(float(fixture["ecdf"][e]) * S) == int(n_lt[e])


def test_ref_reproduces_the_reference_valuations(fixture, ref_on_fixture):
    """Within 4 * 2^-23 * max v + log2(S) * 2^-24 * value: one fp32 ulp each of the reference's exp, of its subtraction and
    of the cast, plus numpy's pairwise fp32 mean."""
    S, E = fixture["log_p"].shape
    M = fixture["strikes"].size
    call = ref_on_fixture["call"][:, :, 0]
    vol = torch.from_numpy(fixture["voltron"].astype(np.float64)).reshape(E, M)
    vmax = ref_on_fixture["vmax"][:, 0]
    worst = 0.0
    for e in range(E):
        for m in range(M):
            bound = scoring_ref.pricer_bound(float(vmax[e]), S, float(call[e, m]))
            err = abs(float(call[e, m]) - float(vol[e, m]))
            worst = max(worst, err / bound)
            assert err <= bound, (e, m, err, bound)
    print("largest |ref - Pricer| / bound:", worst)
    assert float(call.max()) > 30 and float(call.min()) < 1      # the strikes run from deep in to deep out of the money


def test_fixture_records_the_reference_layout(fixture):
    assert list(fixture["columns"]) == ['Expiry', "Strike", "Bid", "Ask", "Voltron", "Return", "ExpClose", "QuoteClose",
                                        "Year", "Sample_Percentile"]
    E, M = fixture["edays"].size, fixture["strikes"].size
    assert fixture["voltron"].shape == (E * M,)
    assert np.array_equal(fixture["strike_col"].reshape(E, M), np.tile(fixture["strikes"], (E, 1)))   # expiry-major rows
    assert list(fixture["expiry_col"].reshape(E, M)[:, 0]) == list(fixture["edays"])
    assert np.array_equal(torch.from_numpy(fixture["log_p"]).exp().numpy(), fixture["pxs"])


def test_crps_identity_against_the_pairwise_form():
    g = torch.Generator().manual_seed(3)
    S = 200
    x = torch.randn(2, S, 3, generator=g)
    truth = torch.randn(2, 3, generator=g)
    for exp in (False, True):
        out = scoring_ref.summarize(x, truth=truth, exp=exp)
        v = x.float().double().exp() if exp else x.float().double()
        for gi in range(2):
            for h in range(3):
                y = float(truth[gi, h])
                want = float(scoring_ref.crps_pairwise(v[gi, :, h], y))
                scale = float(v[gi, :, h].abs().max()) + abs(y)
                assert abs(float(out["crps"][gi, h]) - want) <= 1e-13 * scale


def test_ref_moments_and_quantiles_are_torchs():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 37, 5, generator=g)
    q = torch.linspace(0.05, 0.95, 19, dtype=torch.float64)
    out = scoring_ref.summarize(x, q=q)
    xd = x.double()
    assert torch.allclose(out["moments"][:, 0], xd.mean(1), rtol=0, atol=1e-15)
    assert torch.allclose(out["moments"][:, 1], xd.std(1), rtol=1e-14, atol=0)
    assert torch.equal(out["moments"][:, 2], xd.amin(1)) and torch.equal(out["moments"][:, 3], xd.amax(1))
    assert torch.allclose(out["quant"], torch.quantile(xd, q, dim=1).permute(1, 0, 2), rtol=0, atol=1e-14)
    assert torch.isnan(scoring_ref.summarize(x[:, :1])["moments"][:, 1]).all()          # S = 1: like torch.std


def test_argument_validation_without_a_device():
    from volt_amd import _lib
    L = _lib.lib()
    f = L.volt_path_summary_f32
    nb = L.volt_path_summary_scratch_bytes(2, 100, 5)
    ok = dict(samples=1, ld=5, bs=500, G=2, S=100, H=5, flags=0, q=1, Q=3, truth=None, strikes=1, M=2, moments=1, quant=1,
              counts=1, crps=1, call=1, put=1, scratch=256, scratch_bytes=nb, stream=None)

    def rc(**kw):
        return f(*{**ok, **kw}.values())
    assert rc(samples=None) == -1
    assert rc(ld=4) == -2
    assert rc(G=0) == -4
    assert rc(S=0) == -5 and rc(S=_lib.SUMMARY_MAX_S + 1) == -5
    assert rc(H=0) == -6
    assert rc(flags=2) == -7
    assert rc(q=None) == -8
    assert rc(Q=-1) == -9
    assert rc(strikes=None) == -11
    assert rc(M=-1) == -12
    assert rc(quant=None) == -14
    assert rc(call=None) == -17
    assert rc(put=None) == -18
    assert rc(scratch=None) == -19 and rc(scratch=128) == -19      # missing / not 256-byte aligned
    assert rc(scratch_bytes=nb - 1) == -20
    # (Q = 0 without levels, M = 0 without strikes and a null truth are valid calls: they would LAUNCH, so the GPU tests
    # cover them -- every call above returns before any launch, with or without a device)
    assert _lib.SUMMARY_MAX_S == 32768 and _lib.SUMMARY_EXP == 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "volt_hip.h")).read()
    assert "#define VOLT_SUMMARY_MAX_S 32768" in header and "#define VOLT_SUMMARY_EXP 1" in header


def test_scratch_bytes_formula():
    from volt_amd import _lib
    L = _lib.lib()
    for G, S, H in ((1, 1, 1), (2, 63, 5), (1, 64, 1), (2, 65, 33), (8, 10000, 256), (1, 32768, 2)):
        assert L.volt_path_summary_scratch_bytes(G, S, H) == scoring_ref.scratch_bytes(G, S, H) > 0
        assert scoring_ref.scratch_bytes(G, S, H) == G * H * math.ceil(S / 64) * 256
    for G, S, H in ((0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 32769, 1)):
        assert L.volt_path_summary_scratch_bytes(G, S, H) == 0


def test_no_cpu_fallback_and_shape_errors():
    from volt_amd import ops, option_utils, scoring
    from volt_amd._lib import VoltHipError
    with pytest.raises(VoltHipError):
        scoring.summarize_paths(torch.zeros(10, 3))
    with pytest.raises(VoltHipError):
        ops.path_summary(torch.zeros(1, 10, 3))
    with pytest.raises(VoltHipError):
        option_utils.ECDF(torch.ones(10), torch.tensor(1.0))
    with pytest.raises(ValueError):
        ops.path_summary(torch.zeros(1, ops.SUMMARY_MAX_S + 1, 1))
    with pytest.raises(ValueError):
        scoring.summarize_paths(torch.zeros(10))


def test_calibration_and_gaussian_nll_are_the_notebooks():
    from volt_amd import scoring
    pit = torch.tensor([0.01, 0.2, 0.5, 0.5, 0.96, float("nan")])
    levels = [0.05, 0.5, 0.95]
    got = scoring.calibration(pit, levels)
    known = pit[:5].numpy()
    want = [np.where(known < lv)[0].shape[0] / known.shape[0] for lv in levels]       # Calibration(pcts, level)
    assert np.allclose(got.numpy(), want)
    mean, std, y = torch.tensor([1.0, 2.0]), torch.tensor([0.5, 3.0]), torch.tensor([1.3, -1.0])
    s = scoring.PathSummary(mean=mean, std=std, min=mean, max=mean, quantiles=mean, n_nan=mean, n_lt=mean, n_le=mean,
                            pit=mean, crps=mean, call=mean, put=mean, q=(), nsample=2)
    want = -torch.distributions.Normal(mean, std).log_prob(y)
    assert torch.allclose(scoring.gaussian_nll(s, y), want, rtol=1e-6, atol=1e-6)


def test_driver_keywords_default_to_todays_behaviour():
    from volt_amd import forecast
    from volt_amd.models.Volt import Volt
    for fn in (forecast.GenerateStockPredictionsBatch, forecast.GenerateWindPredictionsBatch, forecast._forecast_windows,
               Volt.Forecast):
        p = inspect.signature(fn).parameters
        assert p["summary"].default is None and p["keep_samples"].default is True, fn.__name__
    with pytest.raises(ValueError):
        forecast._forecast_windows([], torch.zeros(0, 1), [], 1, None, torch.zeros(1), 1, "ewma", 1, 0, 0, 0, None, None,
                                   None, False, None, keep_samples=False)
