"""Host tests of HOW the direct training step is re-issued (eager launches, launch plan, hipGraph): the transitions between the forms.

A recorded plan and a captured graph replay raw device addresses and a stream handle; replaying one after what it addresses was
re-created writes through dangling pointers.  What is pinned here, on the emulated C ABI (tests/abi_emulator.py) and the TINY network
at 8x8, B = 2, Adam, EMA on, grad_norm = 1: a form whose baked identity moved is dropped before it could be replayed, the plan backs
off after going stale 4 times, nothing is built before THIS engine has run one eager step, a recording that cannot be built leaves
the step eager, and the auto-probe measures nothing on the host.  Rows are (step, last_kind, captures, plan is not None, plan_stale,
plan_failed) after each ``Trainer.step``."""
import itertools
import os
import warnings

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from ddpm_torch.utils import train as train_mod
from tests import abi_emulator

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
TINY = dict(in_channels=3, hid_channels=32, out_channels=3, ch_multipliers=[1, 2], num_res_blocks=1, apply_attn=[False, True], drop_rate=0.0)


@pytest.fixture
def emu(monkeypatch):
    return abi_emulator.install(monkeypatch, _hip)


def _trainer(mean_type="eps"):
    torch.manual_seed(0)
    m = ddpm_torch.UNet(**TINY)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), mean_type, "fixed-large", "mse")
    opt = torch.optim.Adam(m.parameters(), lr=2e-4)
    tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, use_ema=True, grad_norm=1.0, shape=(3, 8, 8), device=torch.device("cpu"))
    m.train()
    return m, opt, tr


def _x(i):
    return torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(100 + i)) * 2 - 1


def _ds(tr):
    (ds,) = tr._direct.values()
    return ds


def _steps(tr, first, last, between=None):
    """Steps first..last; rows after each.  ``between``: {step: fn} run BEFORE that step."""
    rows = []
    for i in range(first, last + 1):
        if between and i in between:
            between[i]()
        tr.step(_x(i), global_steps=i)
        ds = _ds(tr)
        rows.append((i, ds.last_kind, ds.captures, ds.plan is not None, ds.plan_stale, ds.plan_failed))
    return rows


def _texts(caught, part):
    return [str(w.message) for w in caught if part in str(w.message)]


def test_identity_churn_backs_off_to_eager_after_four_stale_plans(emu, monkeypatch):
    """Every look at the identity differs from the baked one: each recorded plan is dropped unreplayed, re-recorded three times, then
    given up for good with ONE warning."""
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", "plan")
    tick, identity = itertools.count(), train_mod._DirectStep._identity
    monkeypatch.setattr(train_mod._DirectStep, "_identity", lambda self: identity(self) + (next(tick),))
    m, opt, tr = _trainer()
    rows, settled = [], []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for i in range(1, 10):
            rows += _steps(tr, i, i)
            settled.append(_ds(tr).settled())
    assert rows == [(1, "eager", 0, False, 0, False), (2, "eager", 1, True, 0, False), (3, "eager", 2, True, 1, False),
                    (4, "eager", 3, True, 2, False), (5, "eager", 4, True, 3, False), (6, "eager", 4, False, 4, True),
                    (7, "eager", 4, False, 4, True), (8, "eager", 4, False, 4, True), (9, "eager", 4, False, 4, True)]
    assert len(_texts(caught, "went stale 4 times")) == 1
    assert all(settled)


def _seven_steps_around_a_new_engine(form):
    m, opt, tr = _trainer()
    serials = []
    rows = _steps(tr, 1, 3)
    serials.append(m.engine().serial)
    m.float()                                                     # drops the engine: packed weights, workspaces, staging buffers
    rows += _steps(tr, 4, 7)
    serials.append(m.engine().serial)
    return m, rows, serials


def test_a_new_engine_drops_the_plan_and_warms_up_before_the_next_recording(emu, monkeypatch):
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", "plan")
    m, rows, serials = _seven_steps_around_a_new_engine("plan")
    assert serials[1] > serials[0]
    assert [r[:5] for r in rows] == [(1, "eager", 0, False, 0), (2, "eager", 1, True, 0), (3, "plan", 1, True, 0),
                                     (4, "eager", 1, False, 1),      # the old plan is dropped, the new engine runs its eager step
                                     (5, "eager", 2, True, 1), (6, "plan", 2, True, 1), (7, "plan", 2, True, 1)]
    assert not any(r[5] for r in rows)
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", False)
    m2, rows2, _ = _seven_steps_around_a_new_engine(False)
    assert [r[1:] for r in rows2] == [("eager", 0, False, 0, False)] * 7
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k


def test_a_recording_that_cannot_be_built_leaves_the_step_eager(emu, monkeypatch):
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", "plan")
    record = train_mod.LaunchPlan.record

    def unbuildable(self, body):
        record(self, body)                                        # (the body ran: the step is complete)
        self.build_error = "RuntimeError: injected"
        return self
    monkeypatch.setattr(train_mod.LaunchPlan, "record", unbuildable)
    m, opt, tr = _trainer()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        rows = _steps(tr, 1, 5)
    assert rows == [(1, "eager", 0, False, 0, False)] + [(i, "eager", 0, False, 0, True) for i in range(2, 6)]
    assert len(_texts(caught, "could not be turned into a launch plan")) == 1
    # ... and the steps are the eager ones
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", False)
    m2, opt2, tr2 = _trainer()
    _steps(tr2, 1, 5)
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k


def test_auto_on_the_host_decides_eager_without_measuring(emu, monkeypatch):
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", "auto")
    m, opt, tr = _trainer()
    for i in range(1, 5):
        rows = _steps(tr, i, i)
        ds = _ds(tr)
        assert rows == [(i, "eager", 0, False, 0, False)] and ds.graph is None and not ds.graph_failed
        assert ds.choice == "eager" and ds.times == {} and ds.settled(), i


def _five_steps_with_a_reloaded_optimizer(opt_reload):
    m, opt, tr = _trainer()
    rows = _steps(tr, 1, 3)
    if opt_reload:
        opt.load_state_dict(opt.state_dict())
    rows += _steps(tr, 4, 5)
    return m, rows


def test_reloading_the_optimizers_own_state_does_not_stale_the_plan(emu, monkeypatch):
    """``load_state_dict`` of the optimiser's OWN state dict keeps the moment tensors where they are on the host (no dtype or device to
    change), so the fused update's table and with it the identity stand: pinned so that a change of ``_identity`` is a decision."""
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", "plan")
    m, rows = _five_steps_with_a_reloaded_optimizer(True)
    assert rows == [(1, "eager", 0, False, 0, False), (2, "eager", 1, True, 0, False), (3, "plan", 1, True, 0, False),
                    (4, "plan", 1, True, 0, False), (5, "plan", 1, True, 0, False)]
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", False)
    m2, rows2 = _five_steps_with_a_reloaded_optimizer(True)
    assert [r[1:] for r in rows2] == [("eager", 0, False, 0, False)] * 5
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("forced, mean_type, form", [(False, "eps", "eager"), (True, "eps", "eager"), ("plan", "eps", "plan"),
                                                     ("plan", "x_0", "plan"), ("plan", "mean", "eager")])
def test_form_follows_the_module_attribute_and_what_is_available(emu, monkeypatch, forced, mean_type, form):
    """Forced forms: a hipGraph needs the GPU, so forcing it on the host runs eagerly; a "mean" target gathers its coefficients with
    torch operations a plan cannot see, so it is not plannable and runs eagerly too — without being marked as failed."""
    monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", forced)
    m, opt, tr = _trainer(mean_type)
    rows = _steps(tr, 1, 3)
    ds = _ds(tr)
    assert ds._form() == form
    assert [r[1] for r in rows] == ["eager", "eager", form]
    assert (ds.plan is not None) == (form == "plan") and ds.captures == (1 if form == "plan" else 0)
    assert ds.graph is None and not ds.plan_failed and not ds.graph_failed and ds.plan_stale == 0
