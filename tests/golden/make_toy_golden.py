"""Write fixture G17 (tests/golden/g17_toy_data.pt): the toy datasets, histograms and evaluator of the live reference, to pin
ddpm_torch.toy's data side against upstream's output.  Run where the reference checkout is available:

    python tests/golden/make_toy_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import load_reference as LR  # noqa: E402


def main():
    ref = LR.load()
    spec = importlib.util.spec_from_file_location("ref_toy_data", os.path.join(LR.REFERENCE_ROOT, "ddpm_torch", "toy", "toy_data.py"))
    data_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(data_mod)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {}
    np.random.seed(3)
    g8 = data_mod.Gaussian8(200, random_state=5)
    out["gaussian8"] = dict(np_seed=3, size=200, random_state=5, data=T(g8.data), stdev=float(g8.stdev))
    g25 = data_mod.Gaussian25(200, random_state=5)
    out["gaussian25"] = dict(size=200, random_state=5, data=T(g25.data), stdev=float(g25.stdev))
    sw = data_mod.SwissRoll(200, random_state=5)
    out["swissroll"] = dict(size=200, random_state=5, data=T(sw.data), stdev=T(sw.stdev))
    pts = np.random.default_rng(9).normal(size=(300, 2))
    other = np.random.default_rng(10).normal(0.2, 1.1, size=(300, 2))
    rng = ((-2.0, 2.0), (-1.0, 3.0))
    h1, h2 = ref.functions.hist2d(pts, 12, rng), ref.functions.hist2d(other, "auto", 2.5)
    p, q = h1 / h1.sum(), ref.functions.hist2d(other, 12, rng) / ref.functions.hist2d(other, 12, rng).sum()
    out["hist"] = dict(pts=T(pts), other=T(other), h_pairs=T(h1), h_auto_scalar=T(h2), kl=float(ref.functions.discrete_klv2d(p, q)))
    ev = ref.toy_utils.Evaluator(g25.data, eval_batch_size=50, max_eval_count=200, value_range=(-1.5, 1.5))
    out["evaluator"] = dict(bins=ev.bins, true_hist=T(ev.true_hist))
    torch.save(out, os.path.join(ROOT, "tests", "golden", "g17_toy_data.pt"))


if __name__ == "__main__":
    main()
