"""What the Python layer makes of the rollout kernels' info codes, with rollout_engine.rollout_series replaced by a stub that
returns crafted (samples, info): rollouts_bordered (the public Rollouts route) and forecast._window_pass (the batched
drivers' route) share rollout_engine.report_info.  No device: the mean classes only store their arguments."""
import types
import warnings

import pytest
import torch

from volt_amd import forecast, rollout_engine
from volt_amd.gp import NotPSDError, NumericalWarning
from volt_amd.means import EWMAMean

S, H, N = 6, 4, 12


def _stub(monkeypatch, info):
    calls = []

    def rollout_series(train_x, log_y, log_vol_path, test_x, pred_vol, z, mean_mode, k, *a, **kw):
        G = log_y.shape[0]
        calls.append((mean_mode, k))
        code = torch.as_tensor(info, dtype=torch.int32).reshape(-1, S)
        return torch.arange(G * S * H, dtype=torch.float32).reshape(G, S, H), code.expand(G, S).contiguous()
    monkeypatch.setattr(rollout_engine, "rollout_series", rollout_series)
    return calls


def _model():
    tx = torch.arange(N, dtype=torch.float32) / 252
    prices = torch.linspace(1.0, 2.0, N + 1)
    model = types.SimpleNamespace(mean_module=EWMAMean(tx, prices[1:].log(), 5), log_vol_path=torch.zeros(N),
                                  train_x=tx, train_y=prices[1:].log())
    return tx, prices, (N + torch.arange(H, dtype=torch.float32)) / 252, model


def _bordered(model_args):
    tx, prices, test_x, model = model_args
    return rollout_engine.rollouts_bordered(tx, prices, test_x, model, torch.full((S, H), 0.2), torch.zeros(S, H), None, None)


def test_rollouts_bordered_is_silent_on_a_clean_run_and_mutates_the_model(monkeypatch):
    calls = _stub(monkeypatch, [0] * S)
    args = _model()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = _bordered(args)
    assert calls == [(0, 5)] and tuple(out.shape) == (S, H)
    assert tuple(args[3].train_y.shape) == (S, N + H - 1)               # rollout_utils.py:80-86


def test_rollouts_bordered_warns_with_count_and_first_step_on_positive_info(monkeypatch):
    _stub(monkeypatch, [0, 3, 0, 2, 0, 7])
    with pytest.warns(NumericalWarning) as rec:
        out = _bordered(_model())
    msg = [str(r.message) for r in rec if issubclass(r.category, NumericalWarning)]
    assert len(msg) == 1 and f"3 of {S} sample paths" in msg[0] and "first at horizon step 2)" in msg[0]
    assert tuple(out.shape) == (S, H)


def test_rollouts_bordered_raises_with_count_and_first_step_before_it_mutates_the_model(monkeypatch):
    _stub(monkeypatch, [0, 1, -4, 0, -3, 2])                            # positive codes beside negative ones: it still raises
    args = _model()
    before = (args[3].train_x, args[3].train_y, args[3].log_vol_path, args[3].mean_module.train_y)
    with pytest.raises(NotPSDError, match=rf"2 of {S} sample paths \(first at horizon step 3\)"):
        _bordered(args)
    m = args[3]
    assert all(a is b for a, b in zip((m.train_x, m.train_y, m.log_vol_path, m.mean_module.train_y), before))


def _window(monkeypatch, info, b=2):
    _stub(monkeypatch, info)

    class VolModel:                                                     # the vol forecasters: log pred_vol = 0 everywhere
        def eval(self):
            return self

        def __call__(self, x):
            return types.SimpleNamespace(sample=lambda size: torch.zeros(size[0], b, H))
    monkeypatch.setattr(forecast, "TrainVoltMagpieBatch", lambda *a, **kw: (None, None, None))
    monkeypatch.setattr(forecast, "TrainVolModelBatch", lambda *a, **kw: (VolModel(), None))
    tx = torch.arange(N, dtype=torch.float32) / 252
    test_x = (N + torch.arange(H, dtype=torch.float32)) / 252
    prices = torch.linspace(1.0, 2.0, N + 1).repeat(b, 1)
    return forecast._window_pass(tx, test_x, prices, S, "ewma", 5, 1, 1, 1, None, lambda x, y: torch.full((b, N), 0.2),
                                 None, None)


def test_window_pass_raises_on_negative_info_and_warns_on_positive(monkeypatch):
    """The batched drivers' route reports like the public one (it used to drop info > 0 silently)."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert tuple(_window(monkeypatch, [0] * S).shape) == (2, S, H)
    with pytest.raises(NotPSDError, match=r"2 of 12 sample paths \(first at horizon step 2\)"):
        _window(monkeypatch, [0, 0, -2, 0, 5, 0])
    with pytest.warns(NumericalWarning, match=r"4 of 12 sample paths hit a non-positive pivot \(first at horizon step 1\)"):
        _window(monkeypatch, [0, 1, 0, 0, 5, 0])
