"""CPU: the toy pipeline's host side (ddpm_torch.toy): upstream's parameter layout and seeded init (fixture G8), argument validation of
the toy entry points without a GPU, the datasets, the histogram KL evaluator and the trainer's checkpoint layout."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ddpm_torch import _hip
from ddpm_torch.functions import discrete_klv2d, hist2d
from ddpm_torch.toy import DataStreamer, Decoder, Evaluator, GaussianDiffusion, Trainer, get_beta_schedule
from ddpm_torch.toy.toy_data import Gaussian8, Gaussian25, SwissRoll
from ddpm_torch.utils import infer_range


def test_decoder_state_dict_and_seeded_init_match_upstream(golden):
    g = golden("g8_toy.pt")
    torch.manual_seed(1234)
    m = Decoder(2, 128, 3)
    sd = m.state_dict()
    assert list(sd) == list(g["sd"])                                       # same keys and order, temp_fc.{1,2}.* aliases included
    for k, v in g["sd"].items():
        assert torch.equal(sd[k], v), k
    assert sum(p.numel() for p in m.parameters()) == g["nparams"] == 67074
    m2 = Decoder(2, 128, 3)
    m2.load_state_dict(g["sd"])
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), g["sd"].values()))
    assert m2.temp_fc[0] is m2.temp_fc[2]
    with pytest.raises(RuntimeError, match="CPU"):
        m2(g["x"], g["t"])


@pytest.mark.skipif(not __import__("os").path.exists(_hip.LIB_PATH), reason="libddpm_hip.so not built")
def test_toy_entry_points_validate_on_the_host():
    lib = _hip.lib()
    f = 0x10000                                                            # never dereferenced: every call below is refused before a launch
    assert lib.ddpm_toy_time_table(0, f, f, f, f, f, 100, 128, 0) == 5
    assert lib.ddpm_toy_time_table(f, f, f, f, f, f, 100, 120, 0) == 1     # M not a multiple of 32
    assert lib.ddpm_toy_time_table(f, f, f, f, f, f, 4097, 128, 0) == 1    # T > 4096
    fwd = lambda *geom, x=f: lib.ddpm_toy_decoder_fwd(x, f, *[f] * 12, f, 0, *geom, 0)
    assert fwd(10, 2, 128, 3, 100, x=0) == 5
    assert fwd(10, 17, 128, 3, 100) == 1                                   # D > 16
    assert fwd(10, 2, 288, 3, 100) == 1                                    # M > 256
    assert fwd(10, 2, 128, 0, 100) == 1                                    # L = 0
    assert fwd(0, 2, 128, 3, 100) == 1                                     # B = 0
    assert fwd(2 ** 20, 2, 256, 3, 100) == 1                               # saved buffer past 2 GiB: 32-bit offsets refused
    bwd = lambda B, ws, dy=f: lib.ddpm_toy_decoder_bwd(f, f, dy, *[f] * 10, f, f, 0, f, f, f, ws, B, 2, 128, 3, 100, 0)
    assert bwd(10, 1 << 20, dy=0) == 5
    assert bwd(10, 100) == 1                                               # workspace too small
    assert lib.ddpm_toy_time_table_bwd(f, f, f, f, f, f, f, 3 * 100 * 128 - 1, 10, 128, 100, 0) == 1
    assert lib.ddpm_toy_time_table_bwd(f, 0, f, f, f, f, f, 3 * 100 * 128, 10, 128, 100, 0) == 5


def test_datasets_shapes_and_normalisation():
    np.random.seed(0)
    for cls in (Gaussian8, Gaussian25):
        d = cls(20000, random_state=7)
        assert d.data.shape == (20000, 2) and d.data.dtype == np.float32 and len(d) == 20000
        assert np.allclose(d.data.std(0), 1.0, atol=0.05), d.data.std(0)
        assert torch.is_tensor(d[3]) and d[3].shape == (2,)
    a, b = Gaussian25(100, random_state=3).data, Gaussian25(100, random_state=3).data
    assert np.array_equal(a, b)                                            # noise from default_rng(random_state), modes in turn
    np.random.seed(5); a = Gaussian8(100, random_state=3).data
    np.random.seed(5); b = Gaussian8(100, random_state=3).data
    assert np.array_equal(a, b)                                            # mode choice from the global NumPy RNG
    modes = Gaussian8.scale * np.array(Gaussian8.modes) / Gaussian8(1).stdev
    assert np.abs(a[:, None, :] - modes[None]).min(axis=(1, 2)).max() < 0.2


def test_swissroll_shape_and_scale():
    pytest.importorskip("sklearn")
    d = SwissRoll(20000, random_state=1)
    assert d.data.shape == (20000, 2) and d.data.dtype == np.float32
    assert np.allclose(d.data.std(0), 1.0, atol=0.1), d.data.std(0)


def test_datastreamer_length_iteration_and_resample():
    s = DataStreamer("gaussian8", batch_size=100, num_batches=5)
    assert len(s) == 5 and s.dataset.random_state is None and len(s.dataset) == 500
    batches = list(s)
    assert len(batches) == 5 and all(b.shape == (100, 2) for b in batches)
    assert np.array_equal(torch.cat(batches).numpy(), s.dataset.data)
    first = s.dataset.data.copy()
    list(s)
    assert np.array_equal(first, s.dataset.data)                          # no resampling by default
    r = DataStreamer("gaussian25", batch_size=10, num_batches=3, resample=True)
    before = r.dataset.data.copy()
    list(r)
    assert not np.array_equal(before, r.dataset.data)
    assert DataStreamer.dataset_map("nope") is None


def test_hist2d_and_discrete_kl_against_numpy():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(5000, 2)), rng.normal(0.3, 1.2, size=(5000, 2))
    h = hist2d(a, bins=20, value_range=3)
    assert np.array_equal(h, np.histogram2d(a[:, 0], a[:, 1], bins=20, range=((-3, 3), (-3, 3)))[0])
    assert np.array_equal(hist2d(a, bins=20, value_range=(-2, 2)), np.histogram2d(a[:, 0], a[:, 1], bins=20, range=((-2, 2), (-2, 2)))[0])
    assert np.array_equal(hist2d(a, bins="auto", value_range=((-1, 1), (0, 2))),
                          np.histogram2d(a[:, 0], a[:, 1], bins=math.floor(math.sqrt(500)), range=((-1, 1), (0, 2)))[0])
    p = hist2d(a, 20, 3); p /= p.sum()
    q = hist2d(b, 20, 3); q /= q.sum()
    ref = np.sum(q * (np.log(q + 1e-9) - np.log(p + 1e-9)))
    assert discrete_klv2d(p, q) == pytest.approx(ref, rel=1e-12) and discrete_klv2d(p, q) > 0
    assert discrete_klv2d(p, p) == pytest.approx(0.0, abs=1e-12)


def test_evaluator_kld_of_a_dataset_against_itself_is_zero():
    np.random.seed(1)
    data = Gaussian8(6000, random_state=2).data
    ev = Evaluator(data, eval_batch_size=1000, max_eval_count=6000, value_range=infer_range(Gaussian8(6000, random_state=2)))
    assert ev.bins == math.floor(math.sqrt(600)) and not ev.true_hist.flags.writeable
    chunks = iter([data[i:i + 1000] for i in range(0, 6000, 1000)] + [data[:1000]])
    out = ev.eval(lambda n: next(chunks))
    assert out["x_gen"].shape == (7000, 2)
    assert abs(out["kld"]) < 0.05


def test_toy_trainer_trainees_and_checkpoint_keys(tmp_path):
    torch.manual_seed(0)
    m = Decoder(2, 32, 1)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    dif = GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-large", "mse")
    tr = Trainer(m, opt, dif, epochs=1, trainloader=DataStreamer("gaussian8", 10, 2), chkpt_intv=1)
    assert tr.trainees == ["model", "optimizer", "scheduler"] and tr.shape == (2,)
    path = str(tmp_path / "c.pt")
    tr.save_checkpoint(path, epoch=3, loss=0.5)
    ck = torch.load(path, weights_only=False)
    assert list(ck) == ["model", "optimizer", "scheduler", "epoch", "loss"]
    assert list(ck["model"]) == list(m.state_dict())
    tr2 = Trainer(m, opt, dif, epochs=5, trainloader=DataStreamer("gaussian8", 10, 2))
    tr2.load_checkpoint(path)
    assert tr2.start_epoch == 3


def test_toy_diffusion_never_clips_and_refuses_kl():
    dif = GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-small", "mse")
    assert dif.clip_sampling is False and GaussianDiffusion.__mro__[1].clip_sampling is True
    with pytest.raises(NotImplementedError, match="kl"):
        GaussianDiffusion(get_beta_schedule("linear", 1e-3, 0.2, 100), "eps", "fixed-large", "kl")


def test_toy_data_histograms_and_evaluator_equal_upstream(golden):
    """Fixture G17 (tests/golden/make_toy_golden.py): the reference's own datasets, histograms and evaluator."""
    g = golden("g17_toy_data.pt")
    r = g["gaussian8"]
    np.random.seed(r["np_seed"])
    d = Gaussian8(r["size"], random_state=r["random_state"])
    assert np.array_equal(d.data, r["data"].numpy()) and d.stdev == r["stdev"]
    r = g["gaussian25"]
    d25 = Gaussian25(r["size"], random_state=r["random_state"])
    assert np.array_equal(d25.data, r["data"].numpy()) and d25.stdev == r["stdev"]
    if __import__("importlib").util.find_spec("sklearn") is not None:
        r = g["swissroll"]
        s = SwissRoll(r["size"], random_state=r["random_state"])
        assert np.array_equal(s.stdev, r["stdev"].numpy()) and np.array_equal(s.data, r["data"].numpy())
    h = g["hist"]
    pts, other = h["pts"].numpy(), h["other"].numpy()
    rng = ((-2.0, 2.0), (-1.0, 3.0))
    assert np.array_equal(hist2d(pts, 12, rng), h["h_pairs"].numpy())
    assert np.array_equal(hist2d(other, "auto", 2.5), h["h_auto_scalar"].numpy())
    p, q = hist2d(pts, 12, rng), hist2d(other, 12, rng)
    assert discrete_klv2d(p / p.sum(), q / q.sum()) == pytest.approx(h["kl"], rel=1e-12)
    ev = Evaluator(d25.data, eval_batch_size=50, max_eval_count=200, value_range=(-1.5, 1.5))
    assert ev.bins == g["evaluator"]["bins"] and np.allclose(ev.true_hist, g["evaluator"]["true_hist"].numpy(), rtol=1e-12, atol=0)
