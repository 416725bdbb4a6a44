"""Likelihood CLI of the MI355X build: the negative log-likelihood bound of a checkpoint in bits per dimension, ``L_T + sum_t L_t``
(``GaussianDiffusion.calc_all_bpd``), over ``--total-size`` images of a dataset split.  The reference has no such script (its
``calc_all_bpd`` cannot run); model and checkpoint handling are ``generate.py``'s.

    python eval_bpd.py --dataset cifar10 --chkpt-path chkpts/cifar10/cifar10_2040.pt --split test --save-terms bpd_terms.npz

Prints, and appends to ``metrics.txt`` next to the run's sample folder, the mean total bits/dim, the mean prior term, the mean ``L_0``
and the mean over t of the x_0-estimate MSE; ``--save-terms`` also writes the per-timestep means of both tables.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ddpm_torch  # noqa: E402
import generate  # noqa: E402
from ddpm_torch import datasets  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add = p.add_argument
    add("--config-path", type=str)
    add("--dataset", choices=sorted(ddpm_torch.DATASET_DICT), default="cifar10")
    add("--root", default="~/datasets", type=str)
    add("--split", default="test", type=str, help="dataset split; 'train' / 'all' read through the training transform (random horizontal flip)")
    add("--batch-size", default=128, type=int)
    add("--total-size", default=10000, type=int)
    add("--config-dir", default=os.path.join(HERE, "configs"), type=str)
    add("--chkpt-dir", default="./chkpts", type=str)
    add("--chkpt-path", default="", type=str)
    add("--save-dir", default="./images", type=str, help="as generate.py: metrics.txt goes to <save-dir>/eval/<config>/")
    add("--device", default="cuda:0", type=str)
    add("--use-ema", action="store_true")
    add("--compute", choices=["bf16", "fp32"], default="bf16")
    add("--num-heads", default=1, type=int, help="as generate.py: attention heads, for a config whose model section does not name them")
    add("--num-head-channels", default=0, type=int, help="as generate.py: channels per attention head; 0: use --num-heads")
    add("--clip-denoised", dest="clip_denoised", action="store_true", default=True)
    add("--no-clip-denoised", dest="clip_denoised", action="store_false")
    add("--seed", default=None, type=int, help="seeds the per-step noise of every batch (default: the device's default generator)")
    add("--save-terms", default="", type=str, help="write the per-timestep means of losses and mses ([T] each) to this .npz file")
    args = p.parse_args(argv)
    args.use_ddim, args.num_gpus, args.suffix = False, 1, ""              # what generate.build reads beyond the flags above
    return args


def main(argv=None):
    args = parse_args(argv)
    process, model, device, shape, out_dir = generate.build(args)
    loader, _ = datasets.get_dataloader(args.dataset, batch_size=args.batch_size, split=args.split, val_size=0., root=os.path.expanduser(args.root),
                                        drop_last=False)
    T = process.timesteps
    sums = torch.zeros(3, dtype=torch.float64, device=device)              # total, prior, L_0
    loss_t = torch.zeros(T, dtype=torch.float64, device=device)
    mse_t = torch.zeros(T, dtype=torch.float64, device=device)
    done = batch = 0
    for x in loader:
        x = x[:args.total_size - done].to(device)
        seed = None if args.seed is None else args.seed + batch
        total, losses, prior, mses = process.calc_all_bpd(model, x, clip_denoised=args.clip_denoised, seed=seed)
        sums += torch.stack([total.sum(), prior.sum(), losses[:, 0].sum()]).double()
        loss_t += losses.double().sum(0)
        mse_t += mses.double().sum(0)
        done += len(x)
        batch += 1
        print(f"\r{done}/{args.total_size}", end="", flush=True)
        if done >= args.total_size:
            break
    print()
    if done == 0:
        raise RuntimeError("no images to evaluate")
    sums, loss_t, mse_t = (sums / done).cpu(), (loss_t / done).cpu(), (mse_t / done).cpu()
    result = {"chkpt": os.path.basename(out_dir), "split": args.split, "images": done, "bpd": float(sums[0]), "prior_bpd": float(sums[1]),
              "L_0": float(sums[2]), "mse": float(mse_t.mean())}
    print(f"bits/dim: {result['bpd']:.4f}  (prior {result['prior_bpd']:.3e}, L_0 {result['L_0']:.4f}, mean x_0 MSE {result['mse']:.4e})")
    os.makedirs(os.path.dirname(out_dir), exist_ok=True)
    with open(os.path.join(os.path.dirname(out_dir), "metrics.txt"), "a") as f:
        f.write(str(result) + "\n")
    if args.save_terms:
        np.savez(args.save_terms, losses=loss_t.numpy(), mses=mse_t.numpy())
    return result


if __name__ == "__main__":
    main()
