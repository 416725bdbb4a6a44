"""-m gpu: a bf16 UNet attends over ANY token count (UNet level; the kernels themselves: tests/test_attention_stream_gpu.py).

Before csrc/attention_stream.hip the bf16 mode refused every image whose middle block — which always attends — sees a token count that
is no multiple of 8 (NotImplementedError from _Engine._attn: 24 x 40 with three levels = 60 tokens, 20 x 20 with two = 100), and above
256 tokens it wrote the L x L logits and probabilities to memory.  Here:

  * the reduced network of tests/test_odd_geometry_gpu.py (hid 64, [1, 2, 2], one res block, attention at level 1, dropout 0.1) on
    24 x 40 images, B = 6, train mode: level 1 attends over 240 tokens with the L <= 256 kernels, the middle block over 6 x 10 = 60
    with the streaming pair (12 x 20 and 6 x 10 are rows of launch_replay.ODD_GEOMETRY, so every other layer is known to take them);
    20 x 20 with [1, 2]: 100 tokens at level 1 and in the middle block.  Forward and every parameter gradient against oracle.unet_ref
    with the dropout masks the engine drew, bars of this network family: forward 6e-2 of the oracle's largest output, worst
    per-tensor gradient 5e-2;
  * 32 x 32, hid 64, [1, 2], attention at both levels, B = 2: 1024 tokens at C = 64 and 256 at C = 128; the 1024-token tape record
    holds an lse and no probability tensor; the same net's eval() forward against the oracle;
  * a 4-step ancestral chain on the 24 x 40 net: the graph-replayed loop equals the eager loop bit for bit (the streaming forward is
    captured on its first call: it needs no attribute call or other set-up);
  * three Trainer.steps on the 24 x 40 net as a launch plan and as eager launches (dropout 0, as the config-2 test of the two forms):
    the plan executor has thunks for the two new entry points and replays them."""
import pytest
import torch

import ddpm_torch
from oracle import unet_ref as U
from tests.golden.recipes import rnd
from tests.test_configs_gpu import _grad_report, _masks_from_tape
from tests.test_odd_geometry_gpu import REDUCED
from tests.test_unet_gpu import DEV, make

pytestmark = pytest.mark.gpu
FWD_BAR, GRAD_BAR = 6e-2, 5e-2
TWO_LEVEL = dict(REDUCED, ch_multipliers=[1, 2], apply_attn=[False, True])
LONG = dict(REDUCED, ch_multipliers=[1, 2], apply_attn=[True, True])


def _attn_records(m):
    return [(rec[2].H * rec[2].W, rec[1].in_channels, rec[7], rec[9]) for rec in m.engine().last_tape if rec[0] == "attn"]      # (L, C, prob, lse)


def _train_vs_oracle(cfg, B, H, W):
    m, sd = make(cfg, dtype=torch.bfloat16)
    m.train()
    m.engine().debug_keep_tape = True
    x, gy = rnd(B, 3, H, W, seed=3), rnd(B, 3, H, W, seed=4)
    t = (torch.arange(B) * 47 + 5) % 1000
    y = m(x.to(DEV), t.to(DEV))
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    masks = _masks_from_tape(m, cfg["drop_rate"])
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = U.unet_forward(p, cfg, x, t, training=True, masks=masks)
    (ref * gy).sum().backward()
    rel = float((y.detach().cpu() - ref.detach()).abs().max() / ref.detach().abs().max())
    rows, _ = _grad_report(m, p, 0.1)
    return m, sd, rel, rows


@pytest.mark.parametrize("cfg,B,H,W,tokens", [(REDUCED, 6, 24, 40, {240, 60}), (TWO_LEVEL, 6, 20, 20, {100})],
                         ids=["24x40_three_levels", "20x20_two_levels"])
def test_token_counts_the_bf16_mode_used_to_refuse(cfg, B, H, W, tokens):
    """(on the parent commit: NotImplementedError "attention over 60 tokens in the bf16 mode", raised by the middle block's _attn after
    every earlier layer of the 24 x 40 image had run)"""
    m, _, rel, rows = _train_vs_oracle(cfg, B, H, W)
    recs = _attn_records(m)
    assert {L for L, _, _, _ in recs} == tokens, recs
    assert all(prob is None and lse is not None for _, _, prob, lse in recs), "an attention block materialised its probabilities"
    print(f"\n{H}x{W} B={B} bf16, attention over {[r[0] for r in recs]} tokens: fwd rel {rel:.3e}; worst grads "
          + ", ".join(f"{k}={e:.2e}" for e, k in rows[:4]))
    assert rel < FWD_BAR, rel
    assert rows[0][0] < GRAD_BAR, rows[:4]


def test_1024_tokens_keep_an_lse_and_no_probability_tensor():
    m, sd, rel, rows = _train_vs_oracle(LONG, 2, 32, 32)
    recs = _attn_records(m)
    assert {(L, C) for L, C, _, _ in recs} == {(1024, 64), (256, 128)}, recs
    for L, C, prob, lse in recs:
        assert prob is None and lse is not None and tuple(lse.shape) == (2, L), (L, C)
    print(f"\n32x32 B=2 bf16, attention over 1024 and 256 tokens: fwd rel {rel:.3e}; worst grads " + ", ".join(f"{k}={e:.2e}" for e, k in rows[:4]))
    assert rel < FWD_BAR, rel
    assert rows[0][0] < GRAD_BAR, rows[:4]
    # inference: the streaming forward without an lse
    m.eval()
    x, t = rnd(2, 3, 32, 32, seed=1), torch.tensor([3, 977])
    with torch.no_grad():
        y = m(x.to(DEV), t.to(DEV))
        ref = U.unet_forward(sd, LONG, x, t)
    rel = float((y.cpu() - ref).abs().max() / ref.abs().max())
    print(f"32x32 eval bf16: fwd rel {rel:.3e}")
    assert rel < FWD_BAR, rel


def test_ancestral_chain_24x40_graph_equals_eager(monkeypatch):
    """4 ancestral steps on 24 x 40 images in bf16 (60 tokens in the middle block: the streaming forward with lse = NULL): the
    hipGraph-replayed loop against the eager loop, bit for bit."""
    cfg = dict(REDUCED, drop_rate=0.0)
    m, _ = make(cfg, dtype=torch.bfloat16)
    m.eval()
    steps, shape = 4, (4, 3, 24, 40)
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, steps), "eps", "fixed-large", "mse")
    g = torch.Generator("cpu").manual_seed(31)
    x_T = torch.empty(shape).normal_(generator=g)
    zs = [torch.empty(shape).normal_(generator=g) for _ in range(steps)]
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        with torch.inference_mode():
            outs[mode] = dif._sample_loop(m, shape, DEV, x_T, None, z_stream=iter(zs))
    assert getattr(dif, "_sample_graphs", None), "the sampling step was not captured"
    assert torch.isfinite(outs["1"]).all()
    assert torch.equal(outs["1"], outs["0"]), float((outs["1"] - outs["0"]).abs().max())


def test_three_trainer_steps_24x40_launch_plan_vs_eager(monkeypatch):
    """Trainer.step x 3 (lr 1e-4, clip 1.0, EMA) on the 24 x 40 net, once with step 2 recorded as a launch plan and step 3 replayed by
    csrc/plan.hip, once as eager launches, on the same CPU (t, noise) stream.  The first loss is computed from identical weights by
    the same deterministic forward kernels: equal to fp32 summation noise.  After that the two runs differ by the weight gradients'
    atomic summation order only: Adam moves an element by at most lr per step whatever its gradient, so two runs stay within
    2 lr x steps of each other, and the later losses within a few percent (the bars of the config-2 test of the same two forms)."""
    from ddpm_torch.utils import train as train_mod
    cfg = dict(REDUCED, drop_rate=0.0)
    lr, steps, runs = 1e-4, 3, {}
    for form in ("plan", False):
        monkeypatch.setattr(train_mod, "_TRAIN_GRAPH", form)
        m, _ = make(cfg, dtype=torch.bfloat16)
        m.train()
        dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 1000), "eps", "fixed-large", "mse")
        opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
        tr = ddpm_torch.Trainer(m, opt, dif, epochs=1, trainloader=None, use_ema=True, grad_norm=1.0, shape=(3, 24, 40),
                                device=torch.device(DEV), ema_decay=0.9999)
        gen = torch.Generator("cpu").manual_seed(9)

        def fill(t_buf, noise_buf):
            t_buf.copy_(torch.empty(t_buf.shape, dtype=torch.int64).random_(to=1000, generator=gen))
            noise_buf.copy_(torch.empty(noise_buf.shape).normal_(generator=gen))
        tr.input_source = fill
        losses = []
        for i in range(steps):
            x = torch.rand(6, 3, 24, 40, generator=torch.Generator().manual_seed(40 + i)) * 2 - 1
            tr.stats.reset()
            tr.step(x, global_steps=i + 1)
            losses.append(tr.current_stats["loss"])
        torch.cuda.synchronize()
        ds = next(iter(tr._direct.values()))
        assert ds.last_kind == ("plan" if form == "plan" else "eager")
        assert all(torch.isfinite(p).all() for p in m.parameters())
        runs[form] = (losses, {k: v.detach().float().cpu() for k, v in m.named_parameters()})
    lp, le = runs["plan"][0], runs[False][0]
    worst = max(float((runs["plan"][1][k] - v).abs().max()) for k, v in runs[False][1].items()) / (lr * steps)
    print(f"\n24x40 B=6 bf16: losses launch plan {[round(v, 5) for v in lp]} eager {[round(v, 5) for v in le]}; parameters differ by at most "
          f"{worst:.2f} x lr x steps")
    assert abs(lp[0] - le[0]) <= 1e-5 * abs(le[0])
    assert abs(lp[1] - le[1]) <= 7.5e-3 * abs(le[1]) and abs(lp[2] - le[2]) <= 1.2e-1 * abs(le[2])
    assert worst <= 2.0
