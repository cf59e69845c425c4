"""Path summaries on the device (volt_path_summary_f32, csrc/summary.hip; scoring.py, option_utils.py, the drivers'
``summary=``) against the fp64 yardstick tests/scoring_ref.py on the CPU.

The float tolerance of the general-value tests is derived, not measured: |out - ref| <= 2^-23 |ref| + 2^-36 max|v| over the
column -- one fp32 ulp for the final rounding, and an absolute term for the worst-case fp64 reordering of up to 2^15 terms
and the cancellation in CRPS."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scoring_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
TAIL = 32                      # NaN sentinels behind every output
FLOATS = ("moments", "quant", "crps", "call", "put")


def _raw(samples, q=(), truth=None, strikes=None, exp=False):
    """volt_path_summary_f32 through the C ABI on a device view samples [G,S,H], every output allocated with TAIL NaN (int:
    a magic word) sentinels behind it.  Returns the outputs as CPU tensors after checking the sentinels."""
    from volt_amd import _lib
    L = _lib.lib()
    G, S, H = samples.shape
    sg, ss, sh = samples.stride()
    assert (sh == 1 or H == 1) and (ss >= H or S == 1)
    qd = torch.as_tensor(list(q), dtype=torch.float64).to(DEV)
    Q = qd.numel()
    M = 0 if strikes is None else strikes.shape[1]
    shapes = dict(moments=(G, 4, H), quant=(G, Q, H), counts=(G, 3, H), crps=(G, H), call=(G, M, H), put=(G, M, H))
    bufs = {}
    for name, shape in shapes.items():
        n = int(np.prod(shape))
        if name == "counts":
            bufs[name] = torch.full((n + TAIL,), -777, dtype=torch.int32, device=DEV)
        else:
            bufs[name] = torch.full((n + TAIL,), NAN, dtype=torch.float32, device=DEV)
    nbytes = int(L.volt_path_summary_scratch_bytes(G, S, H))
    assert nbytes == scoring_ref.scratch_bytes(G, S, H)
    scratch = torch.full((nbytes // 4 + 64 + TAIL,), NAN, dtype=torch.float32, device=DEV)
    sp = (scratch.data_ptr() + 255) // 256 * 256
    t = None if truth is None else truth.to(DEV, torch.float32).contiguous()
    k = None if strikes is None else strikes.to(DEV, torch.float32).contiguous()

    def P(x, n=1):
        return None if x is None or n == 0 else x.data_ptr()
    rc = L.volt_path_summary_f32(samples.data_ptr(), ss if S > 1 else H, sg if G > 1 else 0, G, S, H,
                                 _lib.SUMMARY_EXP if exp else 0, P(qd, Q), Q, P(t), P(k, M), M, bufs["moments"].data_ptr(),
                                 P(bufs["quant"], Q), bufs["counts"].data_ptr(), bufs["crps"].data_ptr(), P(bufs["call"], M),
                                 P(bufs["put"], M), sp, nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {}
    for name, shape in shapes.items():
        n = int(np.prod(shape))
        host = bufs[name].cpu()
        if name == "counts":
            assert bool((host[n:] == -777).all()), f"{name}: sentinel overwritten"
        else:
            assert bool(torch.isnan(host[n:]).all()), f"{name}: sentinel overwritten"
        out[name] = host[:n].reshape(shape)
    off = (sp - scratch.data_ptr()) // 4 + nbytes // 4
    assert bool(torch.isnan(scratch[off:].cpu()).all()), "scratch: written past its size"
    return out


def _permutation_columns(G, S, H, offsets=True, seed=0):
    """Every column an independent permutation of 0 .. S-1 (+ 2048 (g H + h)): all values below 2^24."""
    g = torch.Generator().manual_seed(seed)
    x = torch.argsort(torch.rand(G, S, H, generator=g), dim=1).to(torch.float32)
    if offsets:
        x = x + 2048.0 * torch.arange(G * H, dtype=torch.float32).reshape(G, 1, H)
    assert float(x.max()) < 2 ** 24
    return x


def _exact_levels(S):
    """Levels j / (S - 1) with S - 1 a power of two: pos = q (S - 1) is an exact integer in fp64."""
    if S > 1 and (S - 1) & (S - 2) == 0:
        return [j / (S - 1) for j in range(0, S, max(1, (S - 1) // 16))]
    return []


def _check_exact(out, ref, Q):
    for k, name in enumerate(("mean", "std", "min", "max")):
        if name != "std":
            assert torch.equal(out["moments"][:, k], ref["moments"][:, k].float()), name
    assert torch.equal(out["counts"].long(), ref["counts"]), "counts"
    if Q:
        assert torch.equal(out["quant"], ref["quant"].float()), "quant"
    assert not torch.isnan(out["moments"][:, (0, 2, 3)]).any()


EXACT_SHAPES = [(1, 1, 1), (1, 2, 3), (3, 63, 5), (1, 64, 1), (2, 65, 33), (1, 1000, 100), (1, 1025, 7), (2, 4097, 3),
                (1, 32768, 2)]


@pytest.mark.parametrize("G,S,H", EXACT_SHAPES)
def test_exact_on_integer_permutations(G, S, H):
    x = _permutation_columns(G, S, H, offsets=S != 32768, seed=S)
    g = torch.Generator().manual_seed(1)
    pick = torch.randint(0, S, (G, 1, H), generator=g)
    truth = torch.gather(x, 1, pick)[:, 0]                        # one of the column's own values: n_le = n_lt + 1
    strikes = truth[:, :2].mean(-1, keepdim=True).round() + torch.tensor([[-3.0, 0.0, 5.0]])
    q = _exact_levels(S)
    out = _raw(x.to(DEV), q, truth, strikes)
    ref = scoring_ref.summarize(x, q, truth, strikes)
    _check_exact(out, ref, len(q))
    assert torch.equal(out["counts"][:, 2] - out["counts"][:, 1], torch.ones(G, H, dtype=torch.int32))
    # integer data: the option sums are exact too (sums of integers below 2^53, one division, one rounding)
    assert torch.equal(out["call"], ref["call"].float()) and torch.equal(out["put"], ref["put"].float())


def test_exact_without_levels_strikes_or_truth():
    x = _permutation_columns(2, 65, 33, seed=5)
    out = _raw(x.to(DEV))
    ref = scoring_ref.summarize(x)
    _check_exact(out, ref, 0)
    assert bool((out["counts"][:, 1:] == -1).all()) and bool(torch.isnan(out["crps"]).all())


def test_strided_view_in_a_nan_filled_buffer():
    G, S, H, pad, off = 2, 65, 33, 37, 11
    x = _permutation_columns(G, S, H, seed=9)
    big = torch.full((G, S + 3, H + pad), NAN)
    big[:, 1:S + 1, off:off + H] = x
    view = big.to(DEV)[:, 1:S + 1, off:off + H]
    assert view.stride() == ((S + 3) * (H + pad), H + pad, 1) and view.storage_offset() > 0
    q = _exact_levels(S)
    truth = x[:, 7]
    out = _raw(view, q, truth)
    ref = scoring_ref.summarize(x, q, truth)
    _check_exact(out, ref, len(q))
    assert int(out["counts"][:, 0].abs().sum()) == 0
    for name in ("moments", "quant", "crps"):
        sel = out[name] if name != "moments" else out[name][:, (0, 2, 3)]
        assert not torch.isnan(sel).any(), name
    # the same view through the public wrapper (no copy: the strides are passed on)
    from volt_amd import scoring
    s = scoring.summarize_paths(view, q=q, truth=truth)
    assert torch.equal(s.mean.cpu(), out["moments"][:, 0]) and torch.equal(s.n_lt.cpu(), out["counts"][:, 1])
    assert torch.equal(s.quantiles.cpu(), out["quant"])


def test_ties():
    G, S, H = 2, 1000, 7
    g = torch.Generator().manual_seed(11)
    values = torch.tensor([-3.0, 0.0, 2.0, 5.0, 11.0])
    x = values[torch.randint(0, 5, (G, S, H), generator=g)]
    truth = values[torch.randint(0, 5, (G, H), generator=g)]
    out = _raw(x.to(DEV), (), truth)
    mult = (x == truth.unsqueeze(1)).sum(1)
    assert int(mult.min()) > 1
    assert torch.equal((out["counts"][:, 2] - out["counts"][:, 1]).long(), mult)
    assert torch.equal(out["counts"][:, 1].long(), (x < truth.unsqueeze(1)).sum(1))
    assert torch.equal(out["counts"].long(), scoring_ref.summarize(x, (), truth)["counts"])


def _bound_ratios(out, ref):
    """Largest |out - ref| / (2^-23 |ref| + 2^-36 max|v|) per float output."""
    vmax = ref["vmax"]
    ratios = {}
    for name in FLOATS:
        r = ref[name]
        vm = vmax if r.ndim == 2 else vmax.unsqueeze(1)
        bound = 2.0 ** -23 * r.abs() + 2.0 ** -36 * vm
        ratios[name] = float(((out[name].double() - r).abs() / bound).max())
    return ratios


@pytest.mark.parametrize("exp", [False, True])
@pytest.mark.parametrize("S", [50, 1000, 1025, 10000])
def test_general_values_within_the_derived_bound(S, exp):
    G, H, M = 2, 5, 8
    g = torch.Generator().manual_seed(100 + S)
    x = torch.randn(G, S, H, generator=g)
    y = torch.randn(G, H, generator=g)
    truth = y.double().exp().float() if exp else y
    k = torch.randn(G, M, generator=g)
    strikes = k.double().exp().float() if exp else k
    q = [0.05 * j for j in range(1, 20)]
    out = _raw(x.to(DEV), q, truth, strikes, exp)
    ref = scoring_ref.summarize(x, q, truth, strikes, exp)
    assert torch.equal(out["counts"].long(), ref["counts"])
    ratios = _bound_ratios(out, ref)
    print(f"S={S} exp={exp} largest |out - ref| / bound:", {k: round(v, 4) for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r <= 1.0, (name, r)


def test_one_nan_poisons_its_column_only():
    G, S, H = 2, 65, 33
    x = _permutation_columns(G, S, H, seed=21)
    truth = x[:, 3]
    strikes = truth[:, :3].clone()
    q = _exact_levels(S)
    clean = _raw(x.to(DEV), q, truth, strikes)
    xn = x.clone()
    xn[1, 40, 17] = NAN
    out = _raw(xn.to(DEV), q, truth, strikes)
    hit = torch.zeros(G, H, dtype=torch.bool)
    hit[1, 17] = True
    assert int(out["counts"][1, 0, 17]) == 1 and int(out["counts"][1, 1, 17]) == -1 and int(out["counts"][1, 2, 17]) == -1
    for name in FLOATS:
        o, c = out[name], clean[name]
        m = hit if o.ndim == 2 else hit.unsqueeze(1).expand_as(o)
        assert bool(torch.isnan(o[m]).all()), name
        assert torch.equal(o[~m].view(torch.int32), c[~m].view(torch.int32)), name          # bit for bit
    m = hit.unsqueeze(1).expand_as(out["counts"])
    assert torch.equal(out["counts"][~m], clean["counts"][~m])


def test_all_nan_series_and_nan_truth():
    G, S, H = 3, 64, 5
    x = _permutation_columns(G, S, H, seed=23)
    truth = x[:, 9].clone()
    strikes = truth[:, :2].clone()
    clean = _raw(x.to(DEV), (0.5,), truth, strikes)
    xn = x.clone()
    xn[1] = NAN                                                   # what the drivers write for a series whose window failed
    out = _raw(xn.to(DEV), (0.5,), truth, strikes)
    assert bool((out["counts"][1, 0] == S).all()) and bool((out["counts"][1, 1:] == -1).all())
    for name in FLOATS:
        assert bool(torch.isnan(out[name][1]).all()), name
        assert torch.equal(out[name][(0, 2),].view(torch.int32), clean[name][(0, 2),].view(torch.int32)), name
    tn = truth.clone()
    tn[0, 2] = NAN
    tn[2, 4] = NAN
    out = _raw(x.to(DEV), (0.5,), tn, strikes)
    gone = torch.isnan(tn)
    assert bool((out["counts"][:, 1][gone] == -1).all()) and bool((out["counts"][:, 2][gone] == -1).all())
    assert bool(torch.isnan(out["crps"][gone]).all())
    assert torch.equal(out["crps"][~gone].view(torch.int32), clean["crps"][~gone].view(torch.int32))
    assert torch.equal(out["counts"][:, 1:][~gone.unsqueeze(1).expand(G, 2, H)],
                       clean["counts"][:, 1:][~gone.unsqueeze(1).expand(G, 2, H)])
    for name in ("moments", "quant", "call", "put"):
        assert torch.equal(out[name].view(torch.int32), clean[name].view(torch.int32)), name
    assert int(out["counts"][:, 0].abs().sum()) == 0


def test_bitwise_repeatable():
    from volt_amd import scoring
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 1000, 100, generator=g).to(DEV)
    truth = torch.randn(2, 100, generator=g).exp().to(DEV)
    strikes = torch.randn(2, 8, generator=g).exp().to(DEV)
    q = [0.05 * j for j in range(1, 20)]
    first = scoring.summarize_paths(x, q=q, truth=truth, strikes=strikes, exp=True).fields()
    for _ in range(9):
        again = scoring.summarize_paths(x, q=q, truth=truth, strikes=strikes, exp=True).fields()
        for name, t in first.items():
            assert torch.equal(t.view(torch.int32), again[name].view(torch.int32)), name


def test_summarize_paths_matches_the_yardstick_unbatched():
    from volt_amd import scoring
    g = torch.Generator().manual_seed(33)
    x = torch.randn(50, 20, generator=g)
    truth = torch.randn(20, generator=g)
    s = scoring.summarize_paths(x.to(DEV), truth=truth.to(DEV), strikes=torch.tensor([0.0, 1.0]).to(DEV))
    ref = scoring_ref.summarize(x.unsqueeze(0), scoring.DEFAULT_LEVELS, truth.reshape(1, -1), torch.tensor([[0.0, 1.0]]))
    assert s.mean.shape == (20,) and s.quantiles.shape == (5, 20) and s.call.shape == (2, 20) and s.nsample == 50
    assert torch.equal(s.n_lt.cpu().long(), ref["counts"][0, 1]) and torch.equal(s.n_le.cpu().long(), ref["counts"][0, 2])
    assert torch.equal(s.pit.cpu(), ref["counts"][0, 1].float() / 50)
    out = dict(moments=torch.stack((s.mean, s.std, s.min, s.max)).cpu().unsqueeze(0), quant=s.quantiles.cpu().unsqueeze(0),
               crps=s.crps.cpu().unsqueeze(0), call=s.call.cpu().unsqueeze(0), put=s.put.cpu().unsqueeze(0))
    for name, r in _bound_ratios(out, ref).items():
        assert r <= 1.0, (name, r)
    nll = scoring.gaussian_nll(s, truth.to(DEV)).cpu()
    want = -torch.distributions.Normal(x.mean(0), x.std(0)).log_prob(truth)
    assert torch.allclose(nll, want, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        scoring.summarize_paths(torch.zeros(1, 32769, 1, device=DEV))


def test_pricer_and_ecdf_against_the_reference(golden):
    pd = pytest.importorskip("pandas")
    from volt_amd import option_utils
    fx = golden("scoring")
    pxs = torch.from_numpy(fx["pxs"]).to(DEV)
    true_pxs = torch.from_numpy(fx["true_pxs"])
    S, E = fx["pxs"].shape
    edays = [str(e) for e in fx["edays"]]
    rows = [[pd.Timestamp(e), float(k), 1.0 + i, 2.0 + i] for e in edays for i, k in enumerate(fx["strikes"])]
    options = pd.DataFrame(rows, columns=["expiration", "strike", "bid", "ask"])
    df = option_utils.Pricer(pxs, options, edays, true_pxs, float(fx["quote"]))
    assert list(df.columns) == [str(c) for c in fx["columns"]]
    assert np.array_equal(df["Strike"].to_numpy(np.float64), fx["strike_col"])                 # row order
    assert [str(t.date()) for t in df["Expiry"]] == [str(e) for e in fx["expiry_col"]]
    assert np.array_equal(df["Year"].to_numpy(np.int64), fx["year"])
    assert np.array_equal(df["Return"].to_numpy(np.float64), fx["ret"])
    assert np.array_equal(np.round(df["Sample_Percentile"].to_numpy(np.float64) * S), np.round(fx["pct"] * S))
    vmax = float(fx["pxs"].max())
    ours, theirs = df["Voltron"].to_numpy(np.float64), fx["voltron"].astype(np.float64)
    for a, b in zip(ours, theirs):
        assert abs(a - b) <= scoring_ref.pricer_bound(vmax, S, b), (a, b)
    for e in range(E):
        assert option_utils.ECDF(pxs[:, e], true_pxs[e]) == float(fx["ecdf"][e])


def test_drivers_summarise_on_the_device(tmp_path):
    from volt_amd import forecast, scoring
    from volt_amd.synthetic import sde_batch
    B, T, ntrain, H, S = 3, 70, 64, 5, 64
    closes = torch.tensor(sde_batch(B, T - 1, seed=77)[1], dtype=torch.float32, device=DEV)      # [B, T] prices
    names = ["AAA", "BBB", "CCC"]
    strikes = closes[:, ntrain - 1:ntrain] * torch.tensor([0.9, 1.0, 1.1], device=DEV)           # [B, 3]
    spec = scoring.SummarySpec(q=(0.1, 0.5, 0.9), strikes=strikes, exp=True)

    def run(**kw):
        gen = torch.Generator(device=DEV).manual_seed(5)
        torch.manual_seed(5)
        return forecast.GenerateStockPredictionsBatch(names, closes, forecast_horizon=H, train_iters=3, nsample=S,
                                                      ntrain=ntrain, mean="ewma", k=10, ntimes=1, vol_iters=2,
                                                      vol_fn=forecast.realised_vol,
                                                      generator=gen, **kw)
    plain = run()
    samples, summaries = run(summary=spec, save=True, par_dir=str(tmp_path / "a"))
    assert torch.equal(plain.view(torch.int32), samples.view(torch.int32))
    assert len(summaries) == 1
    last_day = ntrain
    truth = closes[:, last_day:last_day + H]
    want = scoring.summarize_paths(samples.to(DEV), q=spec.q, truth=truth, strikes=strikes, exp=True)
    for name, t in want.fields().items():
        assert torch.equal(t.view(torch.int32), summaries[0].fields()[name].view(torch.int32)), name
    assert bool((summaries[0].n_lt >= 0).all())
    files = sorted(p.name for p in (tmp_path / "a" / "AAA").iterdir())
    assert len(files) == 2 and files[1] == files[0][:-3] + "_summary.pt"
    saved = torch.load(str(tmp_path / "a" / "AAA" / files[1]))
    assert torch.equal(saved["mean"], summaries[0].mean[0].cpu())
    none, only = run(summary=spec, keep_samples=False, save=True, par_dir=str(tmp_path / "b"))
    assert none is None
    assert torch.equal(only[0].crps.view(torch.int32), summaries[0].crps.view(torch.int32))
    assert sorted(p.name for p in (tmp_path / "b" / "AAA").iterdir()) == [files[1]]
