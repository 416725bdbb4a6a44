"""CPU, C ABI emulated (tests/abi_emulator.py + tests/inpaint_emulator.py): the host side of inpainting and image editing —
``repaint_schedule``, the jump and previous-level tables, ``GaussianDiffusion.inpaint`` / ``edit`` (``ddim.DDIM`` inherits them), the
``generate.py`` flags — and the argument validation of the two new entry points in the real library.  The kernels themselves are held to
float64 in tests/test_inpaint_gpu.py."""
import glob
import itertools
import json
import os
import sys

import pytest
import torch

import ddpm_torch
from ddpm_torch import _hip
from ddpm_torch.diffusion import repaint_schedule
from oracle import diffusion_ref as D
from tests import abi_emulator, inpaint_emulator
from tests import inpaint_ref as R
from tests.test_abi_surface import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ddpm-torch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
import ddim  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
CPU = torch.device("cpu")
SHAPE = (3, 2, 4, 6)


@pytest.fixture
def emu(monkeypatch):
    return inpaint_emulator.attach(abi_emulator.install(monkeypatch, _hip))


# ------------------------------------------------------------------------------------------------------------------ schedule
def indices(ops, top, j):
    out, i = [top], top
    for op in ops:
        i = i - 1 if op == "down" else i + j
        out.append(i)
    return out


def test_schedule_known_answers_call_counts_and_refusals():
    ops = repaint_schedule(6, jump_length=2, resamples=2)
    assert indices(ops, 5, 2) == [5, 4, 3, 5, 4, 3, 2, 1, 3, 2, 1, 0, -1]
    assert ops.count("down") == 10 and ops.count("up") == 2
    assert repaint_schedule(4, 1, 3).count("down") == 10
    assert repaint_schedule(5) == ["down"] * 5 and repaint_schedule(5, jump_length=3, resamples=1) == ["down"] * 5
    for S, j, r in itertools.product(range(1, 9), range(1, 5), range(1, 4)):
        for start in (None,) + tuple(range(S)):
            top = S - 1 if start is None else start
            if r > 1 and j > top:
                with pytest.raises(ValueError):
                    repaint_schedule(S, j, r, start)
                continue
            ops = repaint_schedule(S, j, r, start)
            assert ops == R.schedule(S, j, r, start), (S, j, r, start)
            assert ops.count("down") == (top + 1) + (r - 1) * j * (top // j) == R.network_calls(S, j, r, start)
            walk = indices(ops, top, j)
            assert walk[-1] == -1 and min(walk[:-1]) >= 0 and max(walk) == top and ops[-1] == "down"
    assert indices(repaint_schedule(6, 2, 2, start=3), 3, 2) == [3, 2, 1, 3, 2, 1, 0, -1]
    for bad in (dict(S=0), dict(S=4, resamples=0), dict(S=4, jump_length=0), dict(S=4, start=4), dict(S=4, start=-1),
                dict(S=4, jump_length=4, resamples=2), dict(S=4, jump_length=2, resamples=2, start=1)):
        with pytest.raises(ValueError):
            repaint_schedule(**bad)


# ------------------------------------------------------------------------------------------------------------------ tables
def bits(a, b):
    """Equal as bit patterns (NaN entries included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def samplers(T=40, size=8):
    betas = ddpm_torch.get_beta_schedule("linear", 1e-4, 0.02, T)
    sub = ddim.get_selection_schedule("linear", size=size, timesteps=T)
    return ddpm_torch.GaussianDiffusion(betas, "eps", "fixed-large", "mse"), ddim.DDIM(betas, "eps", "fixed-small", "mse", eta=0.0, subsequence=sub), betas, sub


def test_previous_level_and_jump_tables_against_float64_closed_forms():
    dif, dd, betas, sub = samplers()
    one = torch.ones(1, dtype=torch.float64)
    for proc, ab in ((dif, torch.cumprod(1.0 - betas, 0)), (dd, torch.cumprod(1.0 - betas, 0)[sub])):
        ab_prev = torch.cat([one, ab[:-1]])
        assert torch.equal(proc.alphas_bar_prev, ab_prev) and torch.equal(proc.sqrt_alphas_bar_prev, torch.sqrt(ab_prev))
        assert torch.equal(proc.sqrt_one_minus_alphas_bar_prev, torch.sqrt(1.0 - ab_prev))
        assert float(proc.sqrt_alphas_bar_prev[0]) == 1.0 and float(proc.sqrt_one_minus_alphas_bar_prev[0]) == 0.0
        alphas = ab / ab_prev
        S = len(ab)
        for j in (1, 2, 3, S - 1):
            ja32, jb32 = proc._jump_tables(j, CPU)
            assert ja32.dtype == torch.float32 and proc._jump_tables(j, CPU)[0] is ja32, "cached per (j, device)"
            ja, jb = getattr(proc, f"repaint_jump_a_{j}"), getattr(proc, f"repaint_jump_b_{j}")
            assert ja.dtype == torch.float64 and bits(ja32, ja.float()) and bits(jb32, jb.float())
            rja, rjb = R.jump_tables(ab, j)
            for i in range(S):
                if i - j < -1:
                    assert ja[i] != ja[i] and jb[i] != jb[i], (i, j)
                    continue
                want = torch.sqrt(torch.prod(alphas[i - j + 1:i + 1]))
                assert abs(float(ja[i] - want)) <= 1e-14 * float(want) and abs(float(ja[i] ** 2 + jb[i] ** 2) - 1.0) <= 1e-15
                assert float(ja[i]) == float(rja[i]) and float(jb[i]) == float(rjb[i])
    # what DDIM had before: the two attributes it used to set itself
    ab = torch.cumprod(1.0 - betas, 0)[sub]
    assert torch.equal(dd.alphas_bar_prev, torch.cat([one, ab[:-1]])) and torch.equal(dd.sqrt_alphas_bar_prev, torch.sqrt(torch.cat([one, ab[:-1]])))


# ------------------------------------------------------------------------------------------------------------------ the loop
def stub(x, t, y=None):
    out = 0.3 * x + 0.01 * t.float().reshape(-1, 1, 1, 1)
    return out if y is None else out + 0.05 * y.float().reshape(-1, 1, 1, 1)


def stub2(x, t):
    return torch.cat([stub(x, t), 0.2 * torch.sin(x)], dim=1)


def draws_for(ops, shape, seed):
    g = torch.Generator().manual_seed(seed)
    n = 1 + sum(2 if op == "down" else 1 for op in ops)
    return [torch.empty(shape).normal_(generator=g) for _ in range(n)]


def half_mask(shape):
    m = torch.zeros(shape[2], shape[3])
    m[:, :shape[3] // 2] = 1
    return m


def source(shape=SHAPE, seed=3):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1)


@pytest.mark.parametrize("which", ["ddpm", "ddim"])
def test_known_region_is_the_source_and_the_chain_follows_the_float64_restatement(emu, which):
    dif, dd, betas, sub = samplers(T=12, size=6)
    proc = dif if which == "ddpm" else dd
    S = proc._num_steps()
    x0, m = source(), half_mask(SHAPE)
    per = torch.stack([m, 1 - m, torch.ones_like(m)])[:, None]                            # a mask per sample
    T64 = R.with_prev(D.ddpm_tables(betas, "fixed-large") if which == "ddpm" else D.ddim_tables(betas, "fixed-small", 0.0, sub))
    for mask, j, r, start in ((m, 2, 2, None), (per, 1, 3, None), (m.bool(), 2, 2, S - 2), (m[None, None], 1, 1, None)):
        ops = repaint_schedule(S, j, r, start)
        dr = draws_for(ops, SHAPE, 5)
        emu.log.clear()
        out = proc.inpaint(stub, x0, mask, jump_length=j, resamples=r, start=start, z_stream=iter(dr))
        assert out.shape == SHAPE and out.dtype == torch.float32
        keep = (torch.as_tensor(mask).float().reshape(-1, 1, SHAPE[2], SHAPE[3]) == 1).expand(SHAPE)
        assert torch.equal(out[keep], x0[keep]), "the known region of the result is the source image"
        assert emu.log.count("ddpm_p_sample_step_masked") == ops.count("down") and emu.log.count("ddpm_q_jump") == ops.count("up")
        ref = R.chain(T64, "eps", None, lambda x, t: stub(x, t), x0.double(), torch.as_tensor(mask).double().reshape(-1, SHAPE[2] * SHAPE[3]),
                      [d.double() for d in dr], j=j, r=r, start=start, timestep_map=None if which == "ddpm" else sub)
        assert float((out.double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), (which, j, r, start)
        assert not torch.equal(out[~keep.expand(SHAPE)], x0[~keep.expand(SHAPE)])


def test_zero_mask_is_the_sampling_loop_and_one_mask_returns_the_source_whatever_the_network_says(emu):
    dif, dd, betas, sub = samplers(T=6, size=3)
    zero, ones = torch.zeros(SHAPE[2], SHAPE[3]), torch.ones(SHAPE[2], SHAPE[3])
    lv = ddpm_torch.GaussianDiffusion(betas, "eps", "learned-range", "hybrid")
    ddlv = ddim.DDIM(betas, "eps", "learned-range", "hybrid", eta=0.5, subsequence=sub)
    for proc, net in ((dif, stub), (dd, stub), (lv, stub2), (ddlv, stub2)):
        S = proc._num_steps()
        dr = draws_for(["down"] * S, SHAPE, 9)
        dr[2::2] = [torch.full(SHAPE, float("nan"))] * S                                    # e is never read under a zero mask
        out = proc.inpaint(net, torch.full(SHAPE, float("nan")), zero, z_stream=iter(dr))
        with torch.inference_mode():
            plain = proc._sample_loop(net, SHAPE, CPU, dr[0], None, z_stream=iter(dr[1::2]))
        assert torch.equal(out, plain) and bool(torch.isfinite(out).all())
        x0 = source()
        nan_net = lambda x, t: torch.full_like(net(x, t), float("nan"))                      # noqa: E731
        assert torch.equal(proc.inpaint(nan_net, x0, ones, seed=1), x0)
    # the launches carry the variance policy and the row pitch of the network output
    n = SHAPE[1] * SHAPE[2] * SHAPE[3]
    modes = {(a[4], a[7]) for a in emu.masked_args}
    assert modes == {(n, 0), (2 * n, 2), (2 * n, 0)}, modes
    assert all(a[:4] == (SHAPE[0], n, SHAPE[2] * SHAPE[3], 1) for a in emu.masked_args)


def test_edit_equals_inpaint_with_a_zero_mask_on_the_same_draws(emu):
    dif, dd, _, _ = samplers(T=8, size=4)
    for proc in (dif, dd):
        S = proc._num_steps()
        for start in (0, S // 2, S - 1):
            x0 = source()
            out = proc.edit(stub, x0, start, seed=11)
            g = torch.Generator().manual_seed(11)                                           # the generator edit seeds: the q_sample draw, then one z per step
            dr = [torch.empty(SHAPE).normal_(generator=g)]
            for _ in range(start + 1):
                dr += [torch.empty(SHAPE).normal_(generator=g), torch.zeros(SHAPE)]
            assert torch.equal(out, proc.inpaint(stub, x0, torch.zeros(SHAPE[2], SHAPE[3]), start=start, z_stream=iter(dr))), start
            assert torch.equal(out, proc.edit(stub, x0, start, seed=11)) and not torch.equal(out, proc.edit(stub, x0, start, seed=12))
        with pytest.raises(ValueError):
            proc.edit(stub, source(), S)
    seen = []
    dif.edit(lambda x, t, y: seen.append(y.clone()) or stub(x, t, y), source(), 2, seed=0, y=torch.tensor([1, 0, 2]))
    assert len(seen) == 3 and all(torch.equal(v, torch.tensor([1, 0, 2])) for v in seen)


def test_rng_order_seed_and_labels(emu):
    dif, _, _, _ = samplers(T=6, size=3)
    x0, m = source(), half_mask(SHAPE)
    ops = repaint_schedule(6, 2, 2)
    dr = draws_for(ops, SHAPE, 21)
    assert len(dr) == 1 + 2 * 10 + 2
    it = iter(dr)
    by_stream = dif.inpaint(stub, x0, m, jump_length=2, resamples=2, z_stream=it)
    assert next(it, None) is None, "the stream is consumed exactly"
    with pytest.raises(StopIteration):
        dif.inpaint(stub, x0, m, jump_length=2, resamples=2, z_stream=iter(dr[:-1]))
    # a seeded run draws the same tensors in the same order: the initial draw, then z, e per reverse step, one draw per jump
    seeded = dif.inpaint(stub, x0, m, jump_length=2, resamples=2, seed=21)
    assert torch.equal(seeded, by_stream)
    assert torch.equal(seeded, dif.inpaint(stub, x0, m, jump_length=2, resamples=2, seed=21))
    assert not torch.equal(seeded, dif.inpaint(stub, x0, m, jump_length=2, resamples=2, seed=22))
    # noise takes the place of the initial draw
    g = torch.Generator().manual_seed(21)
    rest = [torch.empty(SHAPE).normal_(generator=g) for _ in range(22)]
    assert torch.equal(dif.inpaint(stub, x0, m, jump_length=2, resamples=2, seed=21, noise=dr[0]),
                       dif.inpaint(stub, x0, m, jump_length=2, resamples=2, z_stream=iter([dr[0]] + rest)))
    with pytest.raises(ValueError):
        dif.inpaint(stub, x0, m, noise=dr[0], z_stream=iter(dr))
    seen = []
    y = torch.tensor([2, 0, 1])
    out = dif.inpaint(lambda x, t, yy: seen.append(yy.clone()) or stub(x, t, yy), x0, m, seed=3, y=y)
    assert len(seen) == 6 and all(torch.equal(v, y) for v in seen) and not torch.equal(out, dif.inpaint(stub, x0, m, seed=3))
    with pytest.raises(ValueError):
        dif.inpaint(stub, x0, m, y=torch.tensor([0, 1]))
    assert "guidance_scale" not in dif.inpaint.__code__.co_varnames


def test_mask_shape_dtype_and_value_rules(emu):
    dif, _, _, _ = samplers(T=4, size=2)
    x0 = source()
    B, C, H, W = SHAPE
    m = half_mask(SHAPE)
    want = dif.inpaint(stub, x0, m, seed=0)
    for same in (m.bool(), m.to(torch.uint8), m.double(), m.half(), m[None, None], m[None, None].expand(B, 1, H, W), m.numpy()):
        assert torch.equal(dif.inpaint(stub, x0, same, seed=0), want)
    soft = torch.rand(H, W, generator=torch.Generator().manual_seed(0))
    assert bool(torch.isfinite(dif.inpaint(stub, x0, soft, seed=0)).all())
    for bad in (m[None], m[None, None, None], torch.zeros(B, C, H, W), torch.zeros(2, 1, H, W), torch.zeros(W, H), m.reshape(-1)):
        with pytest.raises(ValueError, match="shape"):
            dif.inpaint(stub, x0, bad, seed=0)
    with pytest.raises(ValueError, match="dtype|bool"):
        dif.inpaint(stub, x0, m.long(), seed=0)
    for value in (1.5, -0.1, float("nan"), 255):
        bad = m.clone() if value != 255 else m.to(torch.uint8)
        bad[0, 0] = value
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            dif.inpaint(stub, x0, bad, seed=0)
    with pytest.raises(ValueError):
        dif.inpaint(stub, x0[0], m, seed=0)
    with pytest.raises(ValueError):
        dif.inpaint(stub, x0, m, jump_length=9, resamples=2, seed=0)


# ------------------------------------------------------------------------------------------------------------------ generate.py
TINY_CFG = {
    "dataset": "cifar10",
    "diffusion": {"timesteps": 40, "beta_start": 1e-4, "beta_end": 0.02, "beta_schedule": "linear", "model_mean_type": "eps",
                  "model_var_type": "fixed-large", "loss_type": "mse"},
    "model": {"in_channels": 3, "hid_channels": 32, "ch_multipliers": [1, 2], "num_res_blocks": 1, "apply_attn": [False, True], "drop_rate": 0.1},
    "train": {"lr": 2e-4, "batch_size": 4, "grad_norm": 1.0, "epochs": 1, "warmup": 10, "use_ema": True, "ema_decay": 0.9999},
}


def _files(folder):
    return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(folder, "*.png")))}


def _panel(path, k):
    import numpy as np
    from PIL import Image
    im = np.asarray(Image.open(path))
    return im[2:34, 2 + 34 * k:34 + 34 * k]


def test_generate_inpaint_and_edit_round_trips_and_refusals(emu, tmp_path, monkeypatch):
    import importlib
    import numpy as np
    from PIL import Image
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY_CFG))
    monkeypatch.setenv("DDPM_TORCH_AMD_SYNTHETIC_DATA", "8")
    monkeypatch.chdir(tmp_path)
    importlib.import_module("train").main(["--config-path", str(cfg), "--train-device", "cpu", "--dry-run", "--num-samples", "0", "--num-workers", "0",
                                           "--compute", "fp32", "--chkpt-dir", str(tmp_path / "chk"), "--image-dir", str(tmp_path / "img")])
    chk = str(tmp_path / "chk" / "tiny" / "tiny_1.pt")
    gen = importlib.import_module("generate")
    common = ["--config-path", str(cfg), "--device", "cpu", "--chkpt-path", chk, "--use-ddim", "--subseq-size", "4", "--compute", "fp32"]
    src = tmp_path / "src.pt"
    torch.save(torch.randint(0, 256, (3, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)), src)
    runs = []
    for name in ("a", "b"):
        out = gen.main(common + ["--inpaint", "left", "--source", str(src), "--batch-size", "2", "--seed", "7", "--jump-length", "1", "--resamples", "2",
                                 "--save-dir", str(tmp_path / name)])
        runs.append(_files(out))
    assert sorted(runs[0]) == ["inpaint_00000.png", "inpaint_00001.png", "inpaint_00002.png"] and runs[0] == runs[1]
    first = os.path.join(out, "inpaint_00000.png")
    assert Image.open(first).size == (3 * 34 + 2, 36)                                      # source | masked source | result
    source_, masked, result = (_panel(first, k) for k in range(3))
    assert np.array_equal(source_[:, :16], masked[:, :16]) and np.array_equal(source_[:, :16], result[:, :16])
    assert (masked[:, 16:] == 128).all() and not np.array_equal(source_[:, 16:], result[:, 16:])
    assert "ddpm_p_sample_step_masked" in emu.log and "ddpm_q_jump" in emu.log
    # a mask file, the centre square, and the ancestral sampler's --edit-start
    mfile = tmp_path / "mask.pt"
    torch.save(gen.mask_of("top", (3, 32, 32)), mfile)
    a = _files(gen.main(common + ["--inpaint", str(mfile), "--source", str(src), "--seed", "7", "--save-dir", str(tmp_path / "c")]))
    b = _files(gen.main(common + ["--inpaint", "top", "--source", str(src), "--seed", "7", "--save-dir", str(tmp_path / "d")]))
    assert a == b
    Image.fromarray((gen.mask_of("top", (3, 32, 32)).numpy() * 255).astype(np.uint8)).save(tmp_path / "mask.png")
    assert torch.equal(gen.mask_of(str(tmp_path / "mask.png"), (3, 32, 32)), gen.mask_of("top", (3, 32, 32)))
    c = gen.mask_of("center", (3, 32, 32))
    assert float(c.sum()) == 32 * 32 - 16 * 16 and bool((c[8:24, 8:24] == 0).all())
    for name, kept in (("left", (slice(None), slice(0, 16))), ("right", (slice(None), slice(16, 32))), ("top", (slice(0, 16),)), ("bottom", (slice(16, 32),))):
        mk = gen.mask_of(name, (3, 32, 32))
        assert float(mk.sum()) == 512 and bool((mk[kept] == 1).all())
    out = gen.main(common + ["--edit-start", "2", "--source", str(src), "--seed", "7", "--save-dir", str(tmp_path / "e")])
    assert sorted(_files(out)) == [f"inpaint_{i:05d}.png" for i in range(3)]
    assert Image.open(os.path.join(out, "inpaint_00000.png")).size == (2 * 34 + 2, 36)     # source | result
    # refusals go through parser.error
    for bad in (["--inpaint", "left"], ["--edit-start", "2"],                               # no --source
                ["--use-ddim", "--inpaint", "left", "--source", str(src), "--interpolate", "5"],
                ["--use-ddim", "--inpaint", "left", "--source", str(src), "--reconstruct"],
                ["--inpaint", "left", "--source", str(src), "--labels", "0", "--guidance-scale", "2"],
                ["--edit-start", "2", "--source", str(src), "--labels", "0", "--guidance-scale", "2"]):
        with pytest.raises(SystemExit) as e:
            gen.main(["--config-path", str(cfg), "--device", "cpu", "--chkpt-path", chk] + bad)
        assert e.value.code == 2


# ------------------------------------------------------------------------------------------------------------------ the real library
def test_declarations_agree_and_status_codes_come_back_without_a_gpu():
    """Only refused calls: a call that passes validation would launch on these fake addresses wherever a GPU is present."""
    lib = _hip.lib()
    decl = declared()
    for name, nargs in (("ddpm_p_sample_step_masked", 26), ("ddpm_q_jump", 10)):
        assert decl[name] == nargs == len(_hip.PROTOTYPES[name]) == lib.ddpm_plan_entry_arity(name.encode())
    f = 0x10000
    B, n, hw, T = 2, 24, 8, 50

    def masked(ptrs=None, dims=None, **kw):
        p = dict(x_t=f, model_out=f, z=f, x_known=f, e=f, mask=f, t=f, recip=f, recip_m1=f, c1=f, c2=f, lo=f, hi=f, ka=f, kb=f, x_prev=f)
        d = dict(B=B, n=n, hw=hw, mask_rows=1, out_pitch=n, mean_type=0, clip=1, var_mode=0, T=T)
        p.update({k: v for k, v in kw.items() if k in p})
        d.update({k: v for k, v in kw.items() if k in d})
        return lib.ddpm_p_sample_step_masked(*p.values(), *d.values(), 0)

    for name in ("x_t", "model_out", "z", "x_known", "e", "mask", "t", "recip", "recip_m1", "c1", "c2", "ka", "kb", "x_prev", "lo"):
        assert masked(**{name: 0}) == 5, name
    assert masked(hi=0, var_mode=2, out_pitch=2 * n) == 5 and masked(lo=0, var_mode=2, out_pitch=2 * n) == 5
    for bad in (dict(B=0), dict(n=0), dict(hw=0), dict(T=0), dict(B=-1), dict(B=65536, mask_rows=65536), dict(hw=7), dict(mask_rows=0), dict(mask_rows=3),
                dict(out_pitch=n + 1), dict(out_pitch=3 * n), dict(var_mode=1), dict(var_mode=2), dict(mean_type=-1), dict(mean_type=3), dict(var_mode=3),
                dict(var_mode=-1)):
        assert masked(**bad) == 1, bad
    for name in ("x_t", "model_out", "z", "x_known", "e", "mask", "x_prev"):
        assert masked(**{name: f + 2}) == 3, name
    assert masked(t=f + 4) == 3
    jump = lambda x=f, z=f, t=f, ja=f, jb=f, o=f, B=2, n=8, T=50: lib.ddpm_q_jump(x, z, t, ja, jb, o, B, n, T, 0)      # noqa: E731
    for name in ("x", "z", "t", "ja", "jb", "o"):
        assert jump(**{name: 0}) == 5, name
    for bad in (dict(B=0), dict(n=0), dict(T=0), dict(B=65536), dict(n=-3)):
        assert jump(**bad) == 1, bad
    assert jump(x=f + 1) == 3 and jump(z=f + 2) == 3 and jump(o=f + 3) == 3 and jump(t=f + 4) == 3
