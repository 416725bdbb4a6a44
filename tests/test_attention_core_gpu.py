"""-m gpu: the engine's inference-only attention path ("fused": ddpm_attention_fwd, the L x L tile in LDS and registers), which no other
UNet-level GPU test reaches — it takes one bf16 head over a multiple of 128 tokens above 256 at C = 128 or 256, without a tape.

hid 128, one level, one residual block, attention on, 32 x 16 images (512 tokens at C = 128 in the level's three blocks and the middle
one), B = 2: the eval forward against oracle.unet_ref, and the same network in train mode — where the same blocks stream
(ddpm_attention_stream_*) and the tape says so — under the forward bar tests/test_attention_any_tokens_gpu.py holds this network family to."""
import pytest
import torch

from ddpm_torch import _hip
from oracle import unet_ref as U
from tests.golden.recipes import rnd
from tests.test_attention_any_tokens_gpu import FWD_BAR
from tests.test_unet_gpu import DEV, make

pytestmark = pytest.mark.gpu
CFG = dict(in_channels=3, hid_channels=128, out_channels=3, ch_multipliers=[1], num_res_blocks=1, apply_attn=[True], drop_rate=0.0)


class Names:
    """A launch recorder as _hip.record_into takes one: the entry names, nothing kept alive."""
    retains = False

    def __init__(self):
        self.names = []

    def add(self, name, args):
        self.names.append(name)


def _attention(names):
    return [n for n in names if n.startswith("ddpm_attention") or n.startswith("ddpm_softmax")]


def test_eval_takes_the_fused_kernel_and_training_streams():
    m, sd = make(CFG, dtype=torch.bfloat16)
    x, t, gy = rnd(2, 3, 32, 16, seed=3), torch.tensor([5, 977]), rnd(2, 3, 32, 16, seed=4)
    with torch.no_grad():
        ref = U.unet_forward(sd, CFG, x, t)
    scale = float(ref.abs().max())
    # inference
    m.eval()
    log = Names()
    prev = _hip.record_into(log)
    try:
        with torch.no_grad():
            y = m(x.to(DEV), t.to(DEV))
    finally:
        _hip.record_into(prev)
    rel = float((y.cpu() - ref).abs().max()) / scale
    print(f"\n32x16 B=2 bf16 hid 128, 512 tokens: eval (fused) fwd rel {rel:.3e}")
    assert _attention(log.names) == ["ddpm_attention_fwd"] * 4, _attention(log.names)
    assert rel < FWD_BAR, rel
    # training: the same blocks stream, and the backward runs what the tape names
    m.train()
    m.engine().debug_keep_tape = True
    log = Names()
    prev = _hip.record_into(log)
    try:
        y = m(x.to(DEV), t.to(DEV))
        (y * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        _hip.record_into(prev)
    recs = [r for r in m.engine().last_tape if r[0] == "attn"]
    assert [(r[2].H * r[2].W, r[1].in_channels, r[-1]) for r in recs] == [(512, 128, "stream")] * 4
    assert all(r[7] is None and tuple(r[9].shape) == (2, 512) for r in recs)
    assert _attention(log.names) == ["ddpm_attention_stream_fwd"] * 4 + ["ddpm_attention_stream_bwd"] * 4, _attention(log.names)
    rel = float((y.detach().cpu() - ref).abs().max()) / scale
    print(f"32x16 B=2 bf16 hid 128, 512 tokens: train (stream) fwd rel {rel:.3e}")
    assert rel < FWD_BAR, rel
    assert all(torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in m.parameters())
