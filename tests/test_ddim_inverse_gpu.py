"""-m gpu: DDIM inversion and latent interpolation on the device — `ddpm_ddim_encode_step` and `ddpm_slerp` (csrc/ddim.hip) against
tests/ddim_inverse_ref.py in float64, the encode step against the sampling-step kernel it inverts, `DDIM.encode / reconstruct` through the
engine (replayed against eager, fp32 and bf16 against the oracle UNet in float64), the known-answer chain, and `generate.py --interpolate`.

Every kernel operand sits inside a NaN-filled buffer, every output between sentinel guards that are checked after the launch.

Bars (derived, not measured).  Encode step, per element: 8 * 2^-24 * (|cx x| + |ce eps|) — two products and a sum on fp32-cast tables are
at most three roundings of 2^-24 relative to those magnitudes, a fourth for the cast of the reference, a factor 2 of room; pred_x0 the same
with its own two coefficients.  Slerp, per element: 1e-5 * max(|a_i|, |b_i|) — fixed-order blocked sums are good to log2(n) * 2^-24 = 1e-6
relative, acos is well conditioned away from |c| = 1, a factor 10 of room.
Measured on the MI355X, worst error / bar: encode step 0.246, slerp 0.0164 (details in the docstrings of the tests and DESIGN.md §4);
in the planted slerp cases the orthogonal pair's weights are 3.0e-8 from cos / sin (bar 2.4e-7) and b = a returns a exactly."""
import functools
import glob
import importlib
import json
import math
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from oracle import unet_ref as U
from tests import ddim_inverse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_REAL, S_REAL = 1000, 50
GUARD = 64                       # floats (256 bytes) in front of and behind every embedded operand
SENTINEL = -7777.25
EPS24 = 2.0 ** -24


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def embed(values, offset=0, fill=float("nan")):
    """``values`` inside a ``fill``-filled device buffer, GUARD (+ offset) floats from its 256-byte-aligned base: (buffer, view)."""
    values = values.contiguous()
    buf = torch.full((values.numel() + 2 * GUARD + offset,), fill, dtype=torch.float32, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + values.numel()].view(values.shape)
    view.copy_(values)
    return buf, view


def output(shape, offset=0):
    numel = math.prod(shape)
    buf = torch.full((numel + 2 * GUARD + offset,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD + offset:GUARD + offset + numel].view(shape)


def guards_intact(buf, view, offset=0):
    b = buf.cpu()
    return bool((b[:GUARD + offset] == SENTINEL).all()) and bool((b[GUARD + offset + view.numel():] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def real_tables(schedule):
    """(fp32 device tables in the entry's order, the same tables back in float64) for T = 1000 linear betas, 50 steps."""
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T_REAL)
    tb = R.tables(betas, ddim.get_selection_schedule(schedule, size=S_REAL, timesteps=T_REAL), dtype=torch.float32)
    dev = [tb[k].float().to(DEV) for k in ("cx", "ce", "recip_prev", "recip_m1_prev")]
    return dev, tb


@functools.lru_cache(maxsize=None)
def operands(B, n):
    return r(B, n, seed=11 + n), r(B, n, seed=12 + n)


def launch_encode(schedule, x, eps, t, inplace, want_pred, offset=0):
    """One launch on embedded operands; returns (x_next, pred or None) on the host after checking the guards."""
    tabs, _ = real_tables(schedule)
    B, n = x.shape
    xbuf, xd = embed(x, offset, fill=SENTINEL if inplace else float("nan"))
    _, ed = embed(eps, offset)
    td = t.to(DEV)
    if inplace:
        obuf, od = xbuf, xd
    else:
        obuf, od = output((B, n), offset)
    pbuf, pd = output((B, n), offset) if want_pred else (None, None)
    _hip.call("ddpm_ddim_encode_step", xd.data_ptr(), ed.data_ptr(), td.data_ptr(), *[v.data_ptr() for v in tabs], od.data_ptr(),
              pd.data_ptr() if want_pred else 0, B, n, S_REAL, _hip.stream())
    torch.cuda.synchronize()
    assert guards_intact(obuf, od, offset), "x_next written outside its range"
    if want_pred:
        assert guards_intact(pbuf, pd, offset), "pred_x0 written outside its range"
    if not inplace:
        assert torch.equal(xd.cpu(), x), "x modified by an out-of-place launch"
    return od.cpu(), pd.cpu() if want_pred else None


ENC_WORST = {"x_next": 0.0, "pred_x0": 0.0}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 771, 3072, 196607])
def test_encode_step_kernel_against_float64(n, B):
    """Linear and quadratic 50-step tables (the quadratic one repeats timestep 0: cx = 1, ce = 0 at i = 1, an identity step, which row 2
    takes), in place and out of place, with and without pred_x0, row bases 16-byte aligned where n allows and 4-byte aligned (offset 1).
    Measured on the MI355X: worst error / bar 0.239 (x_next), 0.246 (pred_x0), both at n = 196 607."""
    x, eps = operands(B, n)
    t_sets = [torch.tensor([0]), torch.tensor([S_REAL - 1])] if B == 1 else [torch.tensor([0, S_REAL - 1, 1])]
    for schedule in ("linear", "quadratic"):
        _, tb = real_tables(schedule)
        for t in t_sets:
            want, want_pred = R.encode_step(tb, x, eps, t)
            g = lambda k: tb[k][t][:, None]                                                # noqa: E731
            bar = 8 * EPS24 * ((g("cx") * x.double()).abs() + (g("ce") * eps.double()).abs())
            bar_p = 8 * EPS24 * ((g("recip_prev") * x.double()).abs() + (g("recip_m1_prev") * eps.double()).abs())
            first = None
            for offset in (0, 1):
                for inplace in (False, True):
                    for pred in (False, True):
                        got, got_pred = launch_encode(schedule, x, eps, t, inplace, pred, offset)
                        ratio = float(((got.double() - want).abs() / bar).max())
                        ENC_WORST["x_next"] = max(ENC_WORST["x_next"], ratio)
                        assert ratio <= 1.0, (schedule, t.tolist(), offset, inplace, pred, ratio)
                        if pred:
                            ratio_p = float(((got_pred.double() - want_pred).abs() / bar_p.clamp_min(1e-300)).max())
                            ENC_WORST["pred_x0"] = max(ENC_WORST["pred_x0"], ratio_p)
                            assert ratio_p <= 1.0, (schedule, t.tolist(), offset, inplace, ratio_p)
                        first = got if first is None else first
                        assert torch.equal(got, first), "layouts / repeated launches disagree in bits"
            if schedule == "quadratic" and B == 3:
                assert torch.equal(first[2], x[2]), "the identity step (cx = 1, ce = 0) must return x"
    print(f"\n  n={n} B={B}: worst err/bar so far x_next {ENC_WORST['x_next']:.3f}, pred_x0 {ENC_WORST['pred_x0']:.3f}")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 771, 3072, 196607])
def test_encode_step_out_of_range_t_poisons_its_row_only(n):
    x, eps = operands(3, n)
    good_t = torch.tensor([0, S_REAL - 1, 1])
    good, good_pred = launch_encode("linear", x, eps, good_t, False, True)
    for row, bad in ((1, S_REAL), (2, -1), (0, 2 ** 40)):
        t = good_t.clone()
        t[row] = bad
        for inplace in (False, True):
            got, pred = launch_encode("linear", x, eps, t, inplace, True)
            for b in range(3):
                if b == row:
                    assert bool(torch.isnan(got[b]).all()) and bool(torch.isnan(pred[b]).all())
                else:
                    assert torch.equal(got[b], good[b]) and torch.equal(pred[b], good_pred[b])


def test_encode_step_is_inverted_by_the_sampling_step_kernel():
    """ddpm_p_sample_step(encode_step(x, eps, i), eps, z, t = i, clip = 0) on the product's own DDIM(eta = 0) device tables returns x within
    32 * 2^-24 * (|x| + |eps|) * sqrt(1 / ab[i]) (the decode goes through x_0) at i = 1, 25, 49 and at i = 0, where the kernel masks the
    noise.  z is finite garbage: at eta = 0 its coefficient is exp(0.5 * log 1e-20) = 1e-10.
    Measured on the MI355X: error / bar 0.111, 0.017, 0.0007, 0.095 at i = 1, 25, 49, 0."""
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T_REAL)
    dif = ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=ddim.get_selection_schedule("linear", S_REAL, T_REAL))
    dev = torch.device(DEV)
    enc = [dif._tab(k, dev) for k in ddim._ENCODE_TABLES]
    dec = [dif._tab(k, dev) for k in ddpm_torch.diffusion._STEP_TABLES]
    B, n = 4, 771
    x, eps = operands(B, n)
    z = torch.rand(B, n, generator=torch.Generator().manual_seed(5)) * 2 - 1
    t = torch.tensor([1, 25, 49, 0])
    xd, ed, zd, td = x.to(DEV), eps.to(DEV), z.to(DEV), t.to(DEV)
    nxt, back = torch.empty_like(xd), torch.empty_like(xd)
    _hip.call("ddpm_ddim_encode_step", xd.data_ptr(), ed.data_ptr(), td.data_ptr(), *[v.data_ptr() for v in enc], nxt.data_ptr(), 0, B, n,
              S_REAL, _hip.stream())
    _hip.call("ddpm_p_sample_step", nxt.data_ptr(), ed.data_ptr(), zd.data_ptr(), td.data_ptr(), *[v.data_ptr() for v in dec], back.data_ptr(), 0,
              B, n, 0, 0, S_REAL, _hip.stream())
    ab = dif.alphas_bar[t][:, None]
    bar = 32 * EPS24 * (x.double().abs() + eps.double().abs()) * torch.sqrt(1.0 / ab)
    ratio = ((back.cpu().double() - x.double()).abs() / bar).max(1).values
    print(f"\n  encode -> sampling step, err/bar at i = 1, 25, 49, 0: {[round(float(v), 4) for v in ratio]}")
    assert float(ratio.max()) <= 1.0, ratio


# ------------------------------------------------------------------------------------------------------------------ slerp
def launch_slerp(a, b, al, offset=0):
    P, n = a.shape
    K = len(al)
    _, ad = embed(a, offset)
    _, bd = embed(b, offset)
    _, ald = embed(al)
    obuf, od = output((P, K, n), offset)
    ws_n = int(_hip.lib().ddpm_slerp_workspace_floats(P, n))
    wbuf, wd = output((ws_n,))
    _hip.call("ddpm_slerp", ad.data_ptr(), bd.data_ptr(), ald.data_ptr(), od.data_ptr(), wd.data_ptr(), P, K, n, _hip.stream())
    torch.cuda.synchronize()
    assert guards_intact(obuf, od, offset) and guards_intact(wbuf, wd), "written outside out / ws"
    return od.cpu()


ALPHAS = {1: torch.tensor([0.3]), 2: torch.tensor([0.0, 1.0]), 9: torch.linspace(0, 1, 9)}
SLERP_WORST = [0.0]


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 771, 3072, 196607])
def test_slerp_kernel_against_float64(n, P):
    """Gaussian operands, K = 1, 2 (alpha = 0 and 1), 9; the 16-byte path (n % 4 == 0, aligned) and the element-wise one (odd n, or a base
    4 bytes off).  At n = 1 and 2 the pairs are (anti)parallel or nearly so; the reference applies the same degenerate rule.
    Measured on the MI355X: worst error / bar 0.0164 (n = 196 607, P = 3; bar = 1e-5 * max(|a_i|, |b_i|) per element)."""
    a, b = r(P, n, seed=21 + n), r(P, n, seed=22 + n)
    for K, al in ALPHAS.items():
        want = R.slerp(a, b, al)
        bar = 1e-5 * torch.maximum(a.abs(), b.abs()).double()[:, None, :]
        for offset in (0, 1):
            got = launch_slerp(a, b, al, offset)
            ratio = float(((got.double() - want).abs() / bar).max())
            SLERP_WORST[0] = max(SLERP_WORST[0], ratio)
            assert ratio <= 1.0, (n, P, K, offset, ratio)
            assert torch.equal(got, launch_slerp(a, b, al, offset)), "repeated launches differ"
        if K == 2:
            assert torch.equal(got[:, 0], a) and torch.equal(got[:, 1], b)
    print(f"\n  n={n} P={P}: worst err/bar so far {SLERP_WORST[0]:.4f}")


def test_slerp_planted_cases():
    al = ALPHAS[9]
    n = 3072
    # orthogonal unit vectors: th = pi / 2, the weights are cos / sin of alpha pi / 2
    a, b = torch.zeros(1, n), torch.zeros(1, n)
    a[0, 0], b[0, 2500] = 1.0, 1.0
    got = launch_slerp(a, b, al)
    w0, w1 = torch.cos(al.double() * math.pi / 2), torch.sin(al.double() * math.pi / 2)
    e0, e1 = float((got[0, :, 0].double() - w0).abs().max()), float((got[0, :, 2500].double() - w1).abs().max())
    print(f"\n  orthogonal unit vectors: weight errors {e0:.2e}, {e1:.2e} (bar {4 * EPS24:.2e})")
    assert e0 <= 4 * EPS24 and e1 <= 4 * EPS24
    rest = got.clone()
    rest[0, :, 0], rest[0, :, 2500] = 0.0, 0.0
    assert not rest.any()
    # b = a: the linear branch, every output equals a within 2 ulp
    a = r(1, n, seed=31)
    got = launch_slerp(a, a.clone(), al)
    ulp = torch.nextafter(a.abs(), torch.full_like(a, float("inf"))) - a.abs()
    worst = float(((got - a[:, None]).abs() / ulp[:, None]).max())
    print(f"  b = a: worst distance from a {worst:.2f} ulp")
    assert worst <= 2.0
    # b = -a: the linear branch again, out = (1 - 2 alpha) a
    got = launch_slerp(a, -a, al)
    want = R.slerp(a, -a, al)
    assert float(R.slerp_weights(a, -a, al)[0, 4, 0]) == 0.5                                 # the reference took the linear branch too
    assert float(((got.double() - want).abs() / (1e-5 * a.abs().double()[:, None])).max()) <= 1.0
    assert not got[0, 4].any()                                                             # alpha = 0.5: 0.5 a - 0.5 a
    # a NaN in pair 1 stays in pair 1, at its own element: the pair goes linear, pairs 0 and 2 keep their bits
    a3, b3 = r(3, n, seed=32), r(3, n, seed=33)
    clean = launch_slerp(a3, b3, al)
    a3n = a3.clone()
    a3n[1, 17] = float("nan")
    got = launch_slerp(a3n, b3, al)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    nan = torch.isnan(got[1])
    assert bool(nan[:, 17].all()) and int(nan.sum()) == len(al)
    lin = R.slerp(a3n, b3, al)[1]
    ok = ~torch.isnan(lin)
    assert float(((got[1].double() - lin)[ok].abs()).max()) <= 1e-5 * float(torch.maximum(a3.abs().max(), b3.abs().max()))


def test_slerp_function_shapes_on_the_device():
    a, b = r(2, 3, 8, 8, seed=41).to(DEV), r(2, 3, 8, 8, seed=42).to(DEV)
    out = ddim.slerp(a, b, [0.0, 0.25, 1.0])
    assert out.shape == (2, 3, 3, 8, 8) and out.is_cuda and torch.equal(out[:, 0], a) and torch.equal(out[:, 2], b)
    want = R.slerp(a.cpu(), b.cpu(), torch.tensor([0.0, 0.25, 1.0]))
    assert float((out.cpu().double() - want).abs().max()) <= 1e-5 * float(torch.maximum(a.abs().max(), b.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ through the engine
REDUCED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2, 2], num_res_blocks=1, apply_attn=[False, True, False],
               drop_rate=0.0)
T_SMALL, S_SMALL = 32, 8
# bf16: 2 x the worst error measured on the MI355X over both image sizes, relative to the reference's largest value:
# encode 7.372e-3 (16 x 16; 7.251e-3 at 16 x 48)
BF16_BAR = 1.48e-2


def small_process():
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T_SMALL)
    sub = ddim.get_selection_schedule("linear", size=S_SMALL, timesteps=T_SMALL)
    return ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=sub), betas, sub


@functools.lru_cache(maxsize=None)
def unet_reference(H, W):
    """The oracle UNet in float64 under the float64 restatement, once per image size (shared by the fp32 and the bf16 case)."""
    torch.manual_seed(5)
    m = ddpm_torch.UNet(**REDUCED)
    sd = U.randomize_state_dict(m.state_dict(), 17)
    sd64 = {k: v.double() for k, v in sd.items()}
    x_0 = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W)) * 2 - 1
    _, betas, sub = small_process()
    tb = R.tables(betas, sub)
    net = lambda x, t: U.unet_forward(sd64, REDUCED, x, t)                                 # noqa: E731
    with torch.no_grad():
        latent = R.encode(tb, net, x_0)
        x_rec = R.decode(tb, net, latent)
    return sd, x_0, latent, x_rec


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(16, 16), (16, 48)])
def test_encode_and_reconstruct_through_the_engine(H, W, dtype, monkeypatch):
    """B = 3, T = 32, S = 8 on the reduced UNet.  (a) the replayed encode equals the eager one bit for bit and an encode entry is cached;
    (b) fp32 against the float64 restatement over the oracle UNet, bar 1e-3 of the latent's largest value (the project's fp32 bar);
    (c) bf16 against the same reference, bar 2 x the error measured on the MI355X; (d) fp32 reconstruct against the restatement's own
    reconstruction, same bar as (b) — the round-trip error |x_rec - x_0| is a property of S and the model: printed, not bounded.
    Measured on the MI355X, relative to the reference's largest value: fp32 encode 3.3e-7 (16 x 16) / 3.7e-7 (16 x 48), reconstruct
    1.1e-6 / 1.1e-6; bf16 encode 7.37e-3 / 7.25e-3 (BF16_BAR = 1.48e-2), bf16 reconstruct 1.12e-2 / 1.51e-2 (printed only: the bf16 bar is the
    encoder's).  Round trip max |x_rec - x_0| with these random weights: 0.316 / 0.289 in float64 and fp32, 0.320 / 0.291 in bf16."""
    sd, x_0, want_latent, want_rec = unet_reference(H, W)
    m = ddpm_torch.UNet(**REDUCED)
    m.load_state_dict(sd)
    m.to(DEV).set_compute_dtype(dtype).eval()
    dif, _, _ = small_process()
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        outs[mode] = dif.encode(m, x_0.to(DEV))
        outs[mode + "r"] = dif.reconstruct(m, x_0.to(DEV))
    kinds = [k[3][-1] for k in dif._sample_graphs]
    assert ("encode",) in kinds and ("decode", False) in kinds, kinds
    assert torch.equal(outs["1"], outs["0"]) and outs["1"].is_cuda
    assert all(torch.equal(a, b) for a, b in zip(outs["1r"], outs["0r"])) and torch.equal(outs["1r"][1], outs["1"])
    assert bool(torch.isfinite(outs["1"]).all()) and bool(torch.isfinite(outs["1r"][0]).all())
    e_enc = float((outs["1"].cpu().double() - want_latent).abs().max() / want_latent.abs().max())
    e_rec = float((outs["1r"][0].cpu().double() - want_rec).abs().max() / want_rec.abs().max())
    trip = float((outs["1r"][0].cpu() - x_0).abs().max())
    print(f"\nreduced UNet {H}x{W} {dtype}: encode rel err {e_enc:.3e}, reconstruct rel err {e_rec:.3e}; round trip max |x_rec - x_0| {trip:.3e} "
          f"(float64: {float((want_rec - x_0).abs().max()):.3e})")
    if dtype == torch.float32:
        assert e_enc <= 1e-3 and e_rec <= 1e-3, (e_enc, e_rec)
    else:
        assert e_enc <= BF16_BAR, e_enc


def test_known_answer_chain_on_the_device(monkeypatch):
    """eps = sqrt(1 - alphas_bar[t]) x, S = 50, B = 2, (3, 8, 8): encode and reconstruct are x_0 times the float64 products of the
    per-step gains (round trip 0.998356), replayed and eager.  Bar 1e-5 relative (S * 2^-23 = 6e-6).  Measured on the MI355X: 5.0e-7 (encode) / 1.1e-6 (round trip), the same replayed and eager."""
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T_REAL)
    sub = ddim.get_selection_schedule("linear", S_REAL, T_REAL)
    dif = ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=sub)
    tb = R.tables(betas, sub)
    s64 = torch.sqrt(1.0 - tb["ab"])
    gain = torch.prod(tb["cx"] + tb["ce"] * s64)
    back = torch.prod(tb["coef1"] * (tb["recip"] - tb["recip_m1"] * s64) + tb["coef2"])
    s_dev = torch.sqrt(1.0 - torch.cumprod(1.0 - betas, 0)).float().to(DEV)
    net = lambda x, t: s_dev.index_select(0, t).reshape(-1, 1, 1, 1) * x                   # noqa: E731  (device-side index: capturable)
    x_0 = r(2, 3, 8, 8, seed=50)
    print()
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        x_rec, latent = dif.reconstruct(net, x_0.to(DEV))
        e1 = float((latent.cpu().double() - gain * x_0.double()).abs().max() / (gain * x_0.double()).abs().max())
        e2 = float((x_rec.cpu().double() - gain * back * x_0.double()).abs().max() / x_0.double().abs().max())
        print(f"  graph={mode}: gain {float(gain):.5f} / {float(gain * back):.6f}, rel err encode {e1:.2e}, round trip {e2:.2e}")
        assert e1 <= 1e-5 and e2 <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ generate.py
CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 40, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps",
                  "model_var_type": "fixed-large", "loss_type": "mse"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def test_generate_interpolate_on_the_device(tmp_path, monkeypatch):
    """bf16, tiny configuration: 2 pairs x 5 columns in one chain of 10 rows.  The pictures have the right size, a seeded run repeats byte
    for byte, and columns 0 and K - 1 are the decodes of the two drawn ends (decoded here in a batch of the same size, at the same rows)."""
    import numpy as np
    from PIL import Image
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    train, gen = importlib.import_module("train"), importlib.import_module("generate")
    train.main(["--config-path", str(cfg), "--train-device", DEV, "--dry-run", "--num-samples", "0", "--num-workers", "0", "--compute", "bf16",
                "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    chk = str(tmp_path / "chk" / "tiny" / "tiny_1.pt")
    common = ["--config-path", str(cfg), "--device", DEV, "--chkpt-path", chk, "--use-ddim", "--subseq-size", "4", "--compute", "bf16"]
    K, P = 5, 2
    runs = []
    for name in ("a", "b"):
        out = gen.main(common + ["--interpolate", str(K), "--total-size", str(P), "--batch-size", "10", "--seed", "7", "--save-dir", str(tmp_path / name)])
        files = sorted(glob.glob(os.path.join(out, "*.png")))
        assert [os.path.basename(f) for f in files] == ["interp_00000.png", "interp_00001.png"]
        runs.append([open(f, "rb").read() for f in files])
    assert runs[0] == runs[1]
    pics = [np.asarray(Image.open(f)) for f in files]
    assert all(p.shape == (36, K * 34 + 2, 3) for p in pics) and pics[0].std() > 0
    # the ends, decoded in a batch of the same size at the rows the interpolation put them
    args = gen.parse_args(common + ["--interpolate", str(K)])
    process, model, device, shape, _ = gen.build(args)
    z = torch.randn((2 * P,) + shape, device=device, generator=torch.Generator(device).manual_seed(7))
    batch = torch.zeros((P * K,) + shape, device=device)
    for p in range(P):
        batch[p * K], batch[p * K + K - 1] = z[p], z[P + p]
    ends = gen.to_uint8(process.decode(model, batch).clamp(-1, 1))
    for p in range(P):
        assert (pics[p][2:34, 2:34] == ends[p * K]).all() and (pics[p][2:34, 2 + (K - 1) * 34:2 + (K - 1) * 34 + 32] == ends[p * K + K - 1]).all()
