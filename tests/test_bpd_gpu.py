"""-m gpu: the bits/dim evaluation — `ddpm_bpd_terms` / `ddpm_bpd_finish` (csrc/elementwise.hip) against tests/bpd_ref.py in float64 on the
same fp32 inputs and fp32 tables, and `GaussianDiffusion.calc_all_bpd` end to end (closed-form networks of fixture G18, the reduced UNet
of tests/test_odd_geometry_gpu.py, the toy Decoder), graph-replayed against eager.

Inputs of the kernel tests.  The real T = 1000 linear tables put a decoder of sigma_0 = 0.007 behind t = 0, and in fp32 the discretised
likelihood cdf_upper - cdf_lower is rounding noise against its 1e-12 floor once the model mean is more than ~4 sigma off — a regime in
which the reference's own fp32 arithmetic and float64 disagree by tens of percent, so no kernel could be held to float64 there.  The
network output is therefore the exact target of its parameterisation plus a perturbation that moves the model mean by 0.3 sigma_t per
unit normal (capped at 0.05, the figure of test_variational_bound_term_kernels, which alone still drives the unclipped x_0 estimate of
the eps rows at t = 999 to |x| ~ 30).  Row 0 carries the four tail values of G16 (as far as n allows).

Bars.  losses: max error <= 5e-5 x max |ref| over the tensor (test_variational_bound_term_kernels' form and figure); for n < 16384 —
the layouts that keep vlb_terms_kernel's element order and reduction tree — the values equal ddpm_vlb_terms' bit for bit (the 1024-thread
layout sums 16-byte vectors in another order and is held to the bar alone).  mses, per entry: the larger of 2e-5 x the column's largest
reference value and 8 x the error of an fp32 torch evaluation of the same formulas against float64.
Measured on the MI355X, worst err / bar over every kernel case of this file: losses 0.093 (n = 1, eps), mses 0.212 (n = 2, mean parameterisation, fixed-large); end to end on
fixture G18's networks the mses reach 0.055 of their bar (toy, eps).  The same figures are in DESIGN.md §4 "Evaluation kernels".
"""
import functools
import math

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip, toy
from oracle import diffusion_ref as D
from oracle import toy_ref
from oracle import unet_ref as U
from tests import bpd_ref
from tests.golden.recipes import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_REAL = 1000
NAMES = ("sqrt_recip_alphas_bar", "sqrt_recip_m1_alphas_bar", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_logvar_clipped",
         "fixed_model_logvar")
MEAN_TYPES = ("eps", "x_0", "mean")
WORST = {"losses": 0.0, "mses": 0.0}


def r(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def real_tables(var_type):
    return D.ddpm_tables(D.beta_schedule("linear", 1e-4, 0.02, T_REAL), var_type)


@functools.lru_cache(maxsize=None)
def case(var_type, n, big):
    """Inputs shared by every test of one geometry (never modified): x_0, x_t, t and the three network outputs."""
    tb = real_tables(var_type)
    t = torch.tensor([0, 500] if big else [0, 0, 1, 500, 999, 250])
    B = len(t)
    x0 = (r(B, n, seed=1) * 0.5).clamp(-1, 1)
    tail = torch.tensor([1.0, -1.0, 0.9995, -0.9995])[:min(4, n)]
    x0[0, :len(tail)] = tail
    noise = r(B, n, seed=2)
    f = {k: tb[k].float() for k in tb if torch.is_tensor(tb[k])}
    xt = f["sqrt_alphas_bar"][t][:, None] * x0 + f["sqrt_one_minus_alphas_bar"][t][:, None] * noise
    c1, c2, rm1 = (f[k][t][:, None] for k in ("posterior_mean_coef1", "posterior_mean_coef2", "sqrt_recip_m1_alphas_bar"))
    sigma = torch.exp(0.5 * f["fixed_model_logvar"][t])[:, None]
    pert = r(B, n, seed=7)
    outs = {}
    for mt, target, gain in (("eps", noise, c1 * rm1), ("x_0", x0, c1), ("mean", c1 * x0 + c2 * xt, torch.ones_like(c1))):
        outs[mt] = target + torch.minimum(0.3 * sigma / gain, torch.full_like(sigma, 0.05)) * pert      # gain = |d model mean / d output|
    return dict(t=t, x0=x0, xt=xt, outs=outs, B=B)


def launch_terms(var_type, c, mean_type, clip, decoder, ld, t=None, stream=None, name="ddpm_bpd_terms"):
    """One launch on NaN-filled [B, ld] tables; returns (losses, mses) on the device."""
    tb = real_tables(var_type)
    dev = [v.to(DEV) for v in (c["x0"], c["xt"], c["outs"][MEAN_TYPES[mean_type]], c["t"] if t is None else t)]
    tabs = [tb[k].float().to(DEV) for k in NAMES]
    B, n = c["B"], c["x0"].shape[1]
    if name == "ddpm_vlb_terms":
        loss = torch.full((B,), float("nan"), device=DEV)
        _hip.call(name, *[v.data_ptr() for v in dev + tabs], loss.data_ptr(), 0, B, n, mean_type, clip, T_REAL, _hip.stream())
        return loss
    losses = torch.full((B, ld), float("nan"), device=DEV)
    mses = torch.full((B, ld), float("nan"), device=DEV)
    _hip.call(name, *[v.data_ptr() for v in dev + tabs], losses.data_ptr(), mses.data_ptr(), B, n, ld, mean_type, clip, decoder, T_REAL,
              stream if stream is not None else _hip.stream())
    return losses, mses


def reference(var_type, c, mean_type, clip, decoder, dtype):
    tb = bpd_ref.tables(real_tables(var_type), dtype)
    return bpd_ref.terms(tb, MEAN_TYPES[mean_type], c["x0"].to(dtype), c["xt"].to(dtype), c["t"], c["outs"][MEAN_TYPES[mean_type]].to(dtype),
                         bool(clip), decoder)


def hold(got_l, got_m, ref64, ref32, t, tag):
    """The two bars of the module docstring on the entries a launch addressed (got_*: [B] on the host)."""
    (l64, m64), (_, m32) = ref64, ref32
    err = float((got_l.double() - l64).abs().max()) / (5e-5 * float(l64.abs().max()))
    WORST["losses"] = max(WORST["losses"], err)
    colmax = torch.stack([m64[t == t[b]].max() for b in range(len(t))])
    bar = torch.maximum(2e-5 * colmax, 8 * (m32.double() - m64).abs())
    merr = float(((got_m.double() - m64).abs() / bar).max())
    WORST["mses"] = max(WORST["mses"], merr)
    print(f"  {tag}: losses err/bar {err:.3f}, mses err/bar {merr:.3f}")
    assert err <= 1.0, (tag, "losses", err)
    assert merr <= 1.0, (tag, "mses", merr)


GEOMETRIES = [(n, False) for n in (1, 2, 3, 63, 64, 65, 192, 771, 3072)] + [(196608, True), (196607, True)]


@pytest.mark.parametrize("var_type", ["fixed-small", "fixed-large"])
@pytest.mark.parametrize("n,big", GEOMETRIES, ids=[f"n{n}" for n, _ in GEOMETRIES])
def test_bpd_terms_kernel_against_float64(n, big, var_type):
    """The three layouts (one wave per row up to n = 64, one 256-thread block up to 16 383, 1024 threads with 16-byte loads above), their
    boundaries, and at n = 196 607 a second row whose base is not 16-byte aligned (scalar path); ld = T + 8."""
    c = case(var_type, n, big)
    t, B, ld = c["t"], c["B"], T_REAL + 8
    rows = torch.arange(B)
    print()
    for mean_type in (0, 1, 2):
        for clip in (0, 1):
            vlb = launch_terms(var_type, c, mean_type, clip, 0, ld, name="ddpm_vlb_terms").cpu() if n < 16384 else None
            for decoder in (0, 1):
                losses, mses = (v.cpu() for v in launch_terms(var_type, c, mean_type, clip, decoder, ld))
                written = torch.zeros(B, ld, dtype=torch.bool)
                written[rows, t] = True
                assert torch.equal(~torch.isnan(losses), written) and torch.equal(~torch.isnan(mses), written)      # exactly the addressed entries
                hold(losses[rows, t], mses[rows, t], reference(var_type, c, mean_type, clip, decoder, torch.float64),
                     reference(var_type, c, mean_type, clip, decoder, torch.float32), t, f"n={n} {MEAN_TYPES[mean_type]} clip={clip} dec={decoder}")
                if decoder == 0 and vlb is not None:
                    assert torch.equal(losses[rows, t], vlb), (n, mean_type, clip, (losses[rows, t] - vlb).abs().max())
                elif decoder == 1 and vlb is not None:                       # the decoder only changes the t = 0 rows
                    assert torch.equal(losses[rows, t][t > 0], vlb[t > 0])
    print(f"  worst so far: losses {WORST['losses']:.3f}, mses {WORST['mses']:.3f} of their bars")


@pytest.mark.parametrize("n", [2, 771, 196607])
def test_bpd_terms_out_of_range_t_and_repeatability(n):
    c = case("fixed-large", n, n > 16384)
    B, ld = c["B"], T_REAL + 8
    t_bad = c["t"].clone()
    t_bad[B - 1] = T_REAL                                                     # no column for it: the row stays NaN
    if B > 2:
        t_bad[2] = -1
    losses, mses = (v.cpu() for v in launch_terms("fixed-large", c, 0, 1, 0, ld, t=t_bad))
    ok = (t_bad >= 0) & (t_bad < T_REAL)
    for b in range(B):
        row_l, row_m = ~torch.isnan(losses[b]), ~torch.isnan(mses[b])
        assert int(row_l.sum()) == int(row_m.sum()) == int(ok[b])
        if ok[b]:
            assert bool(row_l[t_bad[b]]) and bool(row_m[t_bad[b]])
    # a second launch, and one on another stream, give the same bits
    a = launch_terms("fixed-large", c, 0, 1, 0, ld)
    b2 = launch_terms("fixed-large", c, 0, 1, 0, ld)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c3 = launch_terms("fixed-large", c, 0, 1, 0, ld, stream=side.cuda_stream)
    torch.cuda.synchronize()
    rows = torch.arange(B)
    for other in (b2, c3):
        for u, v in zip(a, other):
            assert torch.equal(u.cpu()[rows, c["t"]], v.cpu()[rows, c["t"]])


@pytest.mark.parametrize("n", [2, 192, 3072])
def test_bpd_finish_against_float64(n):
    B, T, ld = 3, T_REAL, T_REAL + 8
    tb = real_tables("fixed-large")
    x0 = (r(B, n, seed=3) * 0.5).clamp(-1, 1)
    losses = r(B, ld, seed=4).abs() * 0.01
    losses[:, T:] = float("nan")                                             # the pitch padding is never read
    losses[1, 417] = float("nan")
    prior, total = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    sab, lv = float(tb["sqrt_alphas_bar"][-1].float()), float(torch.log(1 - tb["alphas_bar"][-1]).float())
    x0_d, losses_d = x0.to(DEV), losses.to(DEV)
    _hip.call("ddpm_bpd_finish", x0_d.data_ptr(), losses_d.data_ptr(), prior.data_ptr(), total.data_ptr(), B, n, T, ld, sab, lv, _hip.stream())
    m = torch.tensor(sab, dtype=torch.float32).double() * x0.double()
    lv64 = torch.tensor(lv, dtype=torch.float32).double()
    ref_prior = D.normal_kl(m, lv64, torch.zeros_like(m), torch.zeros_like(m)).mean(1) / math.log(2.0)
    check(prior, bpd_ref.prior_bpd(bpd_ref.tables(tb), x0.double()), 2e-5, name="prior vs tables")
    assert torch.allclose(prior.cpu().double(), ref_prior, rtol=2e-5, atol=0)
    ref_total = losses[:, :T].double().sum(1) + ref_prior
    total = total.cpu()
    assert torch.equal(torch.isnan(total), torch.tensor([False, True, False]))
    assert torch.allclose(total[[0, 2]].double(), ref_total[[0, 2]], rtol=2e-5, atol=0)


# ------------------------------------------------------------------------------------------------------------------ end to end
def hold_all(got, want64, want32, name):
    """The kernel tests' bars on whole results: losses / total 5e-5 x max |ref|, prior 2e-5, mses per entry as in the module docstring."""
    total, losses, prior, mses = (v.cpu() for v in got)
    for k, v in (("total", total), ("losses", losses), ("prior", prior)):
        assert v.dtype == torch.float32 and v.shape == want64[k].shape
        err = float((v.double() - want64[k]).abs().max())
        assert err <= (2e-5 if k == "prior" else 5e-5) * float(want64[k].abs().max()), (name, k, err)
    bar = torch.maximum(2e-5 * want64["mses"].max(0, keepdim=True).values, 8 * (want32["mses"].double() - want64["mses"]).abs())
    merr = float(((mses.double() - want64["mses"]).abs() / bar).max())
    print(f"  {name}: mses err/bar {merr:.3f}")
    assert merr <= 1.0, (name, "mses", merr)


@pytest.mark.parametrize("var_type", ["fixed-small", "fixed-large"])
@pytest.mark.parametrize("mean_type", MEAN_TYPES)
def test_calc_all_bpd_fixture_network_graph_and_eager(golden, monkeypatch, mean_type, var_type):
    """Fixture G18's closed-form network as an arbitrary callable (captured per call), its noise as ``noise_stream``: against the float64
    composition and the fp32 record of the reference; replayed == eager bit for bit; a seed repeats."""
    rec = golden("g18_bpd.pt")["images"]
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule(*rec["schedule"]), mean_type, var_type, "mse")
    tb = bpd_ref.tables(D.ddpm_tables(D.beta_schedule(*rec["schedule"]), var_type))
    w_dev, w64 = rec["w"].to(DEV), rec["w"].double()
    net = lambda x_t, t: 0.7 * x_t + w_dev.index_select(0, t[:1])[0]          # noqa: E731  (device-side index: capturable)
    x_0, noise = rec["x_0"].to(DEV), [z.to(DEV) for z in rec["noise"]]
    print()
    for clip in (True, False):
        want64 = bpd_ref.all_bpd(tb, mean_type, rec["x_0"].double(), rec["noise"].double(), lambda x, t: 0.7 * x + w64[int(t[0])], clip)
        outs = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
            outs[mode] = dif.calc_all_bpd(net, x_0, clip_denoised=clip, noise_stream=iter(noise))
            outs[mode + "s"] = dif.calc_all_bpd(net, x_0, clip_denoised=clip, seed=5)
            again = dif.calc_all_bpd(net, x_0, clip_denoised=clip, seed=5)
            assert all(torch.equal(a, b) for a, b in zip(outs[mode + "s"], again))
        for a, b in zip(outs["1"] + outs["1s"], outs["0"] + outs["0s"]):
            assert a.is_cuda and torch.equal(a, b)
        hold_all(outs["1"], want64, rec["records"][f"{mean_type}/{var_type}/clip{int(clip)}"], f"{mean_type}/{var_type} clip={clip}")


def test_calc_all_bpd_toy_record(golden, monkeypatch):
    rec = golden("g18_bpd.pt")["toy"]
    w_dev, w64 = rec["w"].to(DEV), rec["w"].double()
    print()
    for mean_type in MEAN_TYPES:
        dif = toy.GaussianDiffusion(ddpm_torch.get_beta_schedule(*rec["schedule"]), mean_type, "fixed-large", "mse")
        tb = bpd_ref.tables(D.ddpm_tables(D.beta_schedule(*rec["schedule"]), "fixed-large"))
        want64 = bpd_ref.all_bpd(tb, mean_type, rec["x_0"].double(), rec["noise"].double(), lambda x, t: 0.7 * x + w64[int(t[0])], False, decoder=1)
        outs = []
        for mode in ("1", "0"):
            monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
            outs.append(dif.calc_all_bpd(lambda x_t, t: 0.7 * x_t + w_dev.index_select(0, t[:1])[0], rec["x_0"].to(DEV), noise_stream=iter([z.to(DEV) for z in rec["noise"]])))
        assert all(torch.equal(a, b) for a, b in zip(*outs))
        hold_all(outs[0], want64, rec["records"][f"{mean_type}/fixed-large"], f"toy {mean_type}")


REDUCED = dict(in_channels=3, hid_channels=64, out_channels=3, ch_multipliers=[1, 2, 2], num_res_blocks=1, apply_attn=[False, True, False],
               drop_rate=0.0)
# bf16: 2 x the worst error measured on the MI355X over both image sizes and the four outputs, relative to each output's largest reference
# value: 1.227e-3 (mses at 16 x 16; 1.019e-3 at 16 x 48; losses 4.8e-4 / 5.0e-4, total 3.5e-4 / 2.5e-4, prior <= 8.5e-8)
BF16_BAR = 2.5e-3


@functools.lru_cache(maxsize=None)
def unet_reference(H, W):
    """The oracle UNet composed by bpd_ref on the CPU, once per image size (shared by the fp32 and the bf16 case)."""
    torch.manual_seed(5)
    m = ddpm_torch.UNet(**REDUCED)
    sd = U.randomize_state_dict(m.state_dict(), 17)
    g = torch.Generator().manual_seed(H * 100 + W)
    x_0 = (torch.rand(3, 3, H, W, generator=g) * 2 - 1)
    noise = torch.randn(8, 3, 3, H, W, generator=g)
    tb = D.ddpm_tables(D.beta_schedule("linear", 1e-4, 0.02, 8), "fixed-large")
    with torch.no_grad():
        want = bpd_ref.all_bpd(tb, "eps", x_0, noise, lambda x, t: U.unet_forward(sd, REDUCED, x, t), True)
    return sd, x_0, noise, want


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(16, 16), (16, 48)])
def test_calc_all_bpd_through_the_engine(H, W, dtype, monkeypatch):
    """B = 3, T = 8 on the reduced UNet: the replayed loop against the eager one (bit for bit) and against the oracle UNet under
    bpd_ref on the same noise.  Measured on the MI355X, worst relative error over the four outputs: fp32 2.4e-7 (16 x 16 and 16 x 48,
    losses; bar 1e-3, the project's fp32 bar), bf16 1.23e-3 (16 x 16, mses) / 1.02e-3 (16 x 48, mses); BF16_BAR = 2 x the former."""
    sd, x_0, noise, want = unet_reference(H, W)
    m = ddpm_torch.UNet(**REDUCED)
    m.load_state_dict(sd)
    m.to(DEV).set_compute_dtype(dtype).eval()
    dif = ddpm_torch.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, 8), "eps", "fixed-large", "mse")
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", mode)
        outs[mode] = dif.calc_all_bpd(m, x_0.to(DEV), noise_stream=iter([z.to(DEV) for z in noise]))
    assert any(k[3][2] is not None for k in dif._sample_graphs), "the evaluation step was not captured"
    assert all(torch.equal(a, b) for a, b in zip(outs["1"], outs["0"]))
    errs = {}
    for v, k in zip(outs["1"], ("total", "losses", "prior", "mses")):
        errs[k] = float((v.cpu() - want[k]).abs().max() / want[k].abs().max())
    print(f"\nreduced UNet {H}x{W} {dtype}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    bar = 1e-3 if dtype == torch.float32 else BF16_BAR
    assert max(errs.values()) <= bar, errs


def test_calc_all_bpd_toy_decoder_against_the_oracle(golden, monkeypatch):
    """Decoder(2, 128, 3), T = 100, B = 1000 (the wave-per-row layout, 250 blocks) against oracle/toy_ref.py under bpd_ref."""
    from ddpm_torch.toy import Decoder
    g = golden("g8_toy.pt")
    m = Decoder(2, 128, 3)
    m.load_state_dict(g["sd"])
    m.to(DEV).eval()
    dif = toy.GaussianDiffusion(ddpm_torch.get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-large", "mse")
    gen = torch.Generator().manual_seed(13)
    x_0 = torch.randn(1000, 2, generator=gen)
    noise = [torch.randn(1000, 2, generator=gen) for _ in range(100)]
    monkeypatch.setenv("DDPM_TORCH_AMD_GRAPH", "1")
    got = dif.calc_all_bpd(m, x_0.to(DEV), noise_stream=iter([z.to(DEV) for z in noise]))
    tb = D.ddpm_tables(D.beta_schedule("linear", 1e-3, 0.2, 100), "fixed-large")
    sd = {k: v.clone() for k, v in g["sd"].items()}
    with torch.no_grad():
        want = bpd_ref.all_bpd(tb, "eps", x_0, noise, lambda x, t: toy_ref.decoder_forward(sd, x, t, 128, 3), False, decoder=1)
    for v, k in zip(got, ("total", "losses", "prior", "mses")):
        e = check(v, want[k], 1e-3, name="toy decoder " + k)
        print(f"toy decoder {k}: rel err {e:.3e}")
