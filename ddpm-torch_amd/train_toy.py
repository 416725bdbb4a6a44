"""Training CLI of the 2-D toy pipeline (BASELINE config 1) — counterpart of the reference's ``train_toy.py``: same flags and defaults,
the checkpoint ``<chkpt-dir>/ddpm_<dataset>.pt`` every ``--chkpt-intv`` epochs and a scatter plot of the evaluator's samples under
``<image-dir>/<dataset>/`` every ``--eval-intv`` epochs.  The decoder runs on the GPU kernels only: ``--device`` must name a GPU.

    python train_toy.py --dataset gaussian8 --epochs 100
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from ddpm_torch.toy import DataStreamer, Decoder, Evaluator, GaussianDiffusion, Trainer, get_beta_schedule  # noqa: E402
from ddpm_torch.utils import infer_range, seed_all  # noqa: E402

# flag, type, default, extra argparse keywords
FLAGS = [
    ("dataset", str, "gaussian8", dict(choices=["gaussian8", "gaussian25", "swissroll"])),
    ("size", int, 100000, {}),
    ("root", str, "~/datasets", {}),
    ("epochs", int, 100, {}),
    ("lr", float, 1e-3, {}),
    ("beta1", float, 0.9, {}),
    ("beta2", float, 0.999, {}),
    ("lr-warmup", int, 0, dict(help="epochs of linear learning-rate warm-up")),
    ("batch-size", int, 1000, {}),
    ("timesteps", int, 100, {}),
    ("beta-schedule", str, "linear", dict(choices=["quad", "linear", "warmup10", "warmup50", "jsd"])),
    ("beta-start", float, 1e-3, {}),
    ("beta-end", float, 0.2, {}),
    ("model-mean-type", str, "eps", dict(choices=["mean", "x_0", "eps"])),
    ("model-var-type", str, "fixed-large", dict(choices=["learned", "fixed-small", "fixed-large"])),
    ("loss-type", str, "mse", dict(choices=["kl", "mse"])),
    ("image-dir", str, "./images/train", {}),
    ("chkpt-dir", str, "./chkpts", {}),
    ("chkpt-intv", int, 100, {}),
    ("eval-intv", int, 10, {}),
    ("seed", int, 1234, {}),
    ("device", str, "cuda:0", {}),
    ("mid-features", int, 128, {}),
    ("num-temporal-layers", int, 3, {}),
]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for name, typ, default, extra in FLAGS:
        p.add_argument("--" + name, type=typ, default=default, **extra)
    p.add_argument("--resume", action="store_true", help="continue from <chkpt-dir>/ddpm_<dataset>.pt")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    seed_all(args.seed)
    device = torch.device(args.device)

    stream = DataStreamer(args.dataset, batch_size=args.batch_size, num_batches=args.size // args.batch_size)
    schedule = get_beta_schedule(args.beta_schedule, beta_start=args.beta_start, beta_end=args.beta_end, timesteps=args.timesteps)
    diffusion = GaussianDiffusion(betas=schedule, model_mean_type=args.model_mean_type, model_var_type=args.model_var_type,
                                  loss_type=args.loss_type)
    model = Decoder(2, args.mid_features, args.num_temporal_layers).to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr, betas=(args.beta1, args.beta2))
    warmup = args.lr_warmup
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda e: min((e + 1) / warmup, 1.0)) if warmup > 0 else None

    chkpt_path = os.path.join(args.chkpt_dir, f"ddpm_{args.dataset}.pt")
    image_dir = os.path.join(args.image_dir, args.dataset)
    for d in (args.chkpt_dir, image_dir):
        os.makedirs(d, exist_ok=True)

    trainer = Trainer(model=model, optimizer=optimizer, diffusion=diffusion, epochs=args.epochs, trainloader=stream, scheduler=scheduler,
                      grad_norm=0, device=device, eval_intv=args.eval_intv, chkpt_intv=args.chkpt_intv)

    # samples are scored in one batch of min(size, 30000) points against the stream's first batch (the reference's choice)
    n_eval = min(args.size, 30000)
    xlim, ylim = infer_range(stream.dataset)
    reference = next(iter(stream)).numpy()
    evaluator = Evaluator(true_data=reference, eval_batch_size=n_eval, max_eval_count=n_eval, value_range=(xlim, ylim))

    if args.resume:
        if os.path.exists(chkpt_path):
            trainer.load_checkpoint(chkpt_path)
        else:
            print(f"no checkpoint at {chkpt_path}; starting from scratch")

    trainer.train(evaluator, chkpt_path=chkpt_path, image_dir=image_dir, xlim=xlim, ylim=ylim)


if __name__ == "__main__":
    main()
