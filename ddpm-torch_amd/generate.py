"""Sampling CLI of the MI355X build — counterpart of the reference's ``generate.py`` (tqch/ddpm-torch, ``generate.py:25-178``):
loads a training checkpoint (EMA shadow when the run used EMA, ``module.`` prefixes of DDP runs stripped; a bare state dict
is accepted too), freezes the model and writes ``--total-size`` samples as PNG files, ``--batch-size`` per sampling chain
(ancestral DDPM or ``--use-ddim``).  One process per GPU when ``--num-gpus`` > 1 (independent chains, no exchange).

    python generate.py --dataset cifar10 --chkpt-path chkpts/cifar10/cifar10_2040.pt --use-ddim --total-size 50000

Not in the reference (the deterministic sampler run both ways, ddim.py): ``--interpolate K`` writes one K-column grid per pair of latents
(drawn, or encoded from ``--source``), ``--reconstruct`` writes every ``--source`` image next to its encode -> decode reconstruction and
prints the error.  Both need ``--use-ddim --eta 0``.

    python generate.py --dataset celeba --use-ddim --interpolate 9 --total-size 16 --seed 0
    python generate.py --dataset celeba --use-ddim --reconstruct --source faces.pt

Conditioning a chain on pixels (``GaussianDiffusion.inpaint`` / ``edit``; either sampler): ``--inpaint MASK`` fills the part of every
``--source`` image the mask leaves open (RePaint; ``--jump-length`` / ``--resamples`` for its resampling) and writes source | masked source |
result, ``--edit-start I`` starts the chain from the source noised to index I (SDEdit) and writes source | result.

    python generate.py --dataset celeba --inpaint left --source faces.pt --jump-length 10 --resamples 10 --seed 0
    python generate.py --dataset celeba --use-ddim --edit-start 20 --source faces.pt
"""
import argparse
import json
import math
import os
import sys
import uuid
from concurrent.futures import ThreadPoolExecutor

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ddim  # noqa: E402
import ddpm_torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add = p.add_argument
    add("--config-path", type=str)
    add("--dataset", choices=sorted(ddpm_torch.DATASET_DICT), default="cifar10")
    add("--batch-size", default=128, type=int)
    add("--total-size", default=50000, type=int)
    add("--config-dir", default=os.path.join(HERE, "configs"), type=str)
    add("--chkpt-dir", default="./chkpts", type=str)
    add("--chkpt-path", default="", type=str)
    add("--save-dir", default="./images", type=str)
    add("--device", default="cuda:0", type=str)
    add("--use-ema", action="store_true")
    add("--use-ddim", action="store_true")
    add("--eta", default=0., type=float)
    add("--skip-schedule", default="linear", type=str)
    add("--subseq-size", default=50, type=int)
    add("--suffix", default="", type=str)
    add("--max-workers", default=8, type=int)
    add("--num-gpus", default=1, type=int)
    add("--compute", choices=["bf16", "fp32"], default="bf16")
    add("--seed", default=None, type=int, help="seeds x_T AND the per-step noise of every chain (default: nondeterministic, like the reference)")
    add("--num-heads", default=1, type=int, help="attention heads of the model, for a config whose model section names neither num_heads nor "
        "num_head_channels (the section wins; no checkpoint records the head count)")
    add("--num-head-channels", default=0, type=int, help="channels per attention head instead of a head count; 0: use --num-heads")
    add("--labels", default="", type=str, help="class-conditional checkpoints: the classes to generate, a comma list repeated over the images "
        "(\"3,5\") or \"cycle\" for 0, 1, ..., K-1 repeated; K is read off the checkpoint's class_embed.weight.  Default: the null class")
    add("--guidance-scale", default=1.0, type=float, help="classifier-free guidance scale w of w * out(x, y) + (1 - w) * out(x, null) "
        "(Ho & Salimans 2022); 1 = plain conditional sampling; needs --labels; learned-variance models take 1 only")
    add("--interpolate", default=0, type=int, metavar="K", help="write K-step spherical interpolations between pairs of latents (--total-size "
        "pairs of drawn latents, or the consecutive pairs of --source), one grid picture per pair; needs --use-ddim --eta 0")
    add("--reconstruct", action="store_true", help="encode every --source image and decode it again; writes input | reconstruction and prints "
        "the mean squared error per dimension on the [0, 1] scale (Song et al. 2020, Table 2)")
    add("--source", default="", type=str, help="images for --interpolate / --reconstruct / --inpaint / --edit-start: a tensor file ([N, C, H, W], "
        "uint8 or float in [-1, 1]) or a folder of pictures at the dataset's resolution")
    add("--inpaint", default="", type=str, metavar="MASK", help="fill the masked region of every --source image: left | right | top | bottom "
        "(keep that half), center (generate the central half-side square), or a tensor / image file holding the mask (1 = keep, 0 = generate)")
    add("--jump-length", default=1, type=int, metavar="J", help="--inpaint: levels a RePaint chain jumps back up before it comes down again")
    add("--resamples", default=1, type=int, metavar="R", help="--inpaint: times every stretch of J levels is walked (1 = no jump)")
    add("--edit-start", default=None, type=int, metavar="I", help="start the chain from every --source image noised to index I (SDEdit); "
        "with --inpaint: where the inpainting chain starts")
    args = p.parse_args(argv)
    if args.inpaint or args.edit_start is not None:
        what = "--inpaint" if args.inpaint else "--edit-start"
        if not args.source:
            p.error(f"{what} requires --source")
        if args.interpolate or args.reconstruct:
            p.error(f"{what} and --interpolate / --reconstruct are separate runs")
        if args.guidance_scale != 1.0:
            p.error(f"{what} samples at --guidance-scale 1")
        if args.num_gpus > 1:
            p.error(f"{what} runs on one GPU")
        if args.jump_length < 1 or args.resamples < 1:
            p.error("--jump-length and --resamples are at least 1")
    elif args.interpolate or args.reconstruct:
        what = "--interpolate" if args.interpolate else "--reconstruct"
        if not args.use_ddim or args.eta != 0:
            p.error(f"{what} runs the deterministic sampler both ways: it requires --use-ddim --eta 0")
        if args.interpolate and args.reconstruct:
            p.error("--interpolate and --reconstruct are separate runs")
        if args.interpolate < 0 or args.interpolate == 1:
            p.error("--interpolate K needs K >= 2 columns")
        if args.reconstruct and not args.source:
            p.error("--reconstruct requires --source")
        if args.num_gpus > 1:
            p.error(f"{what} runs on one GPU")
    elif args.source:
        p.error("--source is read by --interpolate, --reconstruct, --inpaint and --edit-start only")
    if args.guidance_scale != 1.0 and not args.labels:
        p.error("--guidance-scale guides towards the classes of --labels")
    if args.labels and (args.interpolate or args.reconstruct):
        p.error("--labels serves plain generation: --interpolate and --reconstruct run unconditionally (the null class)")
    return args


def weights_from(chkpt, prefer_ema):
    """The state dict to sample with: EMA shadow / model section of a training checkpoint, or the file itself."""
    try:
        sd = chkpt["ema"]["shadow"] if prefer_ema else chkpt["model"]
    except (KeyError, TypeError):
        print("Not a training checkpoint: loading it directly as model weights...")
        sd = chkpt
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def build(args, rank=0):
    path = args.config_path or os.path.join(args.config_dir, args.dataset + ".json")
    with open(path) as f:
        meta = json.load(f)
    dataset = meta.get("dataset", args.dataset)
    info = ddpm_torch.DATASET_INFO[dataset]
    shape = (info["channels"], info["resolution"][0], info["resolution"][0])
    dk = dict(meta["diffusion"])
    betas = ddpm_torch.get_beta_schedule(dk.pop("beta_schedule"), dk.pop("beta_start"), dk.pop("beta_end"), dk.pop("timesteps"))
    learned = dk.get("model_var_type") in ("learned", "learned-range")        # the network emits 2C channels: mean output | v
    if args.use_ddim:
        if not learned:                                                       # (DDIM itself takes the mean half of a learned-variance model)
            dk["model_var_type"] = "fixed-small"
        sub = ddim.get_selection_schedule(args.skip_schedule, size=args.subseq_size, timesteps=len(betas))
        process = ddim.DDIM(betas, **dk, eta=args.eta, subsequence=sub)
    else:
        process = ddpm_torch.GaussianDiffusion(betas, **dk)
    device = torch.device(f"cuda:{rank}" if args.num_gpus > 1 else args.device)
    mk = dict(meta["model"])
    block = mk.pop("block_size", 1)
    mk["in_channels"] = mk.get("in_channels", info["channels"]) * block ** 2
    chkpt_path = args.chkpt_path or os.path.join(args.chkpt_dir, f"ddpm_{dataset}.pt")
    use_ema = meta.get("train", {}).get("use_ema", args.use_ema)
    weights = weights_from(torch.load(chkpt_path, map_location=device), use_ema)
    table = next((v for k, v in weights.items() if k.endswith("class_embed.weight")), None)
    mk["num_classes"] = None if table is None else table.shape[0] - 1          # the checkpoint decides: one row per class + the null class
    # ... and so it does for the scale-shift norm: a ResidualBlock's fc then has 2 * Cout rows, Cout being its conv1's
    fc = next(((v, weights.get(k[:-len("fc.weight")] + "conv1.weight")) for k, v in weights.items() if k.endswith(".fc.weight")), None)
    mk["use_scale_shift_norm"] = bool(fc is not None and fc[1] is not None and fc[0].shape[0] == 2 * fc[1].shape[0])
    # (the head count changes no parameter: no checkpoint can tell it, so the config — or, for a config without the keys, the flags — must)
    ddpm_torch.UNet.head_options(mk, getattr(args, "num_heads", 1), getattr(args, "num_head_channels", 0))
    model = ddpm_torch.UNet(out_channels=(2 if learned else 1) * info["channels"] * block ** 2, **mk).set_compute_dtype(args.compute)
    if block > 1:
        model = ddpm_torch.ModelWrapper(model, torch.nn.PixelUnshuffle(block), torch.nn.PixelShuffle(block))
    model.to(device)
    model.load_state_dict(weights)
    model.eval()
    for prm in model.parameters():
        prm.requires_grad_(False)
    exp = os.path.splitext(os.path.basename(path))[0]
    out_dir = os.path.join(args.save_dir, "eval", exp, os.path.splitext(os.path.basename(chkpt_path))[0] + args.suffix)
    return process, model, device, shape, out_dir


def to_uint8(x):
    """[-1, 1] float NCHW -> uint8 NHWC (generate.py:129)."""
    return (x * 127.5 + 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def write_png(arr, out_dir):
    from PIL import Image
    Image.fromarray(arr.squeeze(-1) if arr.shape[-1] == 1 else arr).save(os.path.join(out_dir, f"{uuid.uuid4()}.png"))


def labels_of(spec, num_classes, start, n, device):
    """int64 [n] class labels of images ``start`` ... ``start + n - 1`` of a run: ``spec`` is "cycle" (0, 1, ..., K-1 repeated) or a comma
    list repeated over the images."""
    if num_classes is None:
        raise ValueError("--labels needs a class-conditional checkpoint (one with class_embed.weight)")
    pattern = list(range(num_classes)) if spec.strip() == "cycle" else [int(v) for v in spec.split(",") if v.strip()]
    if not pattern or min(pattern) < 0 or max(pattern) >= num_classes:
        raise ValueError(f"--labels {spec!r}: expected classes in [0, {num_classes})")
    idx = (torch.arange(n) + start) % len(pattern)
    return torch.tensor(pattern, dtype=torch.int64)[idx].to(device)


def generate(rank, args):
    process, model, device, shape, out_dir = build(args, rank)
    os.makedirs(out_dir, exist_ok=True)
    world = max(args.num_gpus, 1)
    mine = args.total_size // world + (1 if rank < args.total_size % world else 0)
    first = rank * (args.total_size // world) + min(rank, args.total_size % world)          # index of this rank's first image in the run
    num_classes = next((m.num_classes for m in model.modules() if getattr(m, "num_classes", None) is not None), None)
    done = chain = 0
    with ThreadPoolExecutor(max_workers=args.max_workers) as pool:
        while done < mine:
            n = min(args.batch_size, mine - done)
            cond = {}
            if args.labels:
                cond = {"y": labels_of(args.labels, num_classes, first + done, n, device), "guidance_scale": args.guidance_scale}
            if args.seed is None:                    # the reference's behaviour (generate.py:126-128): x_T and every z from the default RNG
                x = process.p_sample(model, shape=(n,) + shape, device=device, noise=torch.randn((n,) + shape, device=device), **cond)
            else:
                # reproducible runs: ONE seeded generator per chain feeds x_T and then every per-step z (diffusion.py:164-171), so the
                # whole chain — not only its starting point — repeats; chains and ranks get distinct streams
                x = process.p_sample(model, shape=(n,) + shape, device=device, seed=args.seed + 1000003 * rank + chain, **cond)
            chain += 1
            list(pool.map(lambda a: write_png(a, out_dir), list(to_uint8(x))))
            done += n
            if rank == 0:
                print(f"\r{done}/{mine}", end="", flush=True)
    if rank == 0:
        print()
    return out_dir


def load_source(path, shape):
    """``--source`` as float32 [N, C, H, W] in [-1, 1]: a tensor file (uint8 is mapped like the data sets', x / 127.5 - 1; float is taken as
    it is) or a folder of pictures of exactly the dataset's resolution, in name order."""
    if os.path.isdir(path):
        import numpy as np
        from PIL import Image
        names = sorted(f for f in os.listdir(path) if f.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
        if not names:
            raise ValueError(f"--source {path}: no pictures in this folder")
        imgs = []
        for f in names:
            im = Image.open(os.path.join(path, f)).convert("L" if shape[0] == 1 else "RGB")
            if im.size != (shape[2], shape[1]):
                raise ValueError(f"--source {os.path.join(path, f)}: {im.size[0]} x {im.size[1]}, the dataset is {shape[2]} x {shape[1]}")
            arr = torch.from_numpy(np.asarray(im).copy())
            imgs.append(arr[None] if arr.ndim == 2 else arr.permute(2, 0, 1))
        x = torch.stack(imgs)
    else:
        x = torch.load(path, map_location="cpu")
        if not torch.is_tensor(x):
            raise ValueError(f"--source {path}: expected a tensor, got {type(x).__name__}")
    if x.ndim != 4 or tuple(x.shape[1:]) != tuple(shape):
        raise ValueError(f"--source {path}: shape {tuple(x.shape)}, expected [N, {shape[0]}, {shape[1]}, {shape[2]}]")
    return x.float() / 127.5 - 1.0 if x.dtype == torch.uint8 else x.float()


def invert(args):
    """--interpolate / --reconstruct: deterministic file names (interp_00000.png, recon_00000.png, ...), so a seeded run repeats byte for byte."""
    from ddpm_torch.utils import save_image_grid
    process, model, device, shape, out_dir = build(args)
    os.makedirs(out_dir, exist_ok=True)
    src = load_source(args.source, shape) if args.source else None
    if args.reconstruct:
        sq = done = 0
        for i in range(0, len(src), args.batch_size):
            x = src[i:i + args.batch_size].to(device)
            x_rec, _ = process.reconstruct(model, x)
            sq += float((((x_rec - x) / 2) ** 2).double().sum())
            for j in range(len(x)):
                save_image_grid(torch.stack([x[j], x_rec[j]]), os.path.join(out_dir, f"recon_{done + j:05d}.png"), nrow=2)
            done += len(x)
        print(f"reconstruction error of {done} images (mean squared error per dimension, [0, 1] scale): {sq / (done * src[0].numel()):.6f}")
        return out_dir
    K = args.interpolate
    pairs = len(src) // 2 if src is not None else args.total_size
    per_chain = max(1, args.batch_size // K)                   # a chain decodes per_chain * K <= --batch-size rows (one pair at the least)
    done = chain = 0
    while done < pairs:
        p = min(per_chain, pairs - done)
        if src is not None:
            ends = src[2 * done:2 * (done + p)].to(device)
            x = process.interpolate(model, ends[0::2], ends[1::2], num=K, batch_size=args.batch_size)
        else:
            rng = torch.Generator(device)
            if args.seed is not None:
                rng.manual_seed(args.seed + chain)
            else:
                rng.seed()
            z = torch.randn((2 * p,) + shape, device=device, generator=rng)
            x = process.interpolate(model, z[:p], z[p:], num=K, encoded=True, batch_size=args.batch_size)
        for j in range(p):
            save_image_grid(x[j], os.path.join(out_dir, f"interp_{done + j:05d}.png"), nrow=K)
        done += p
        chain += 1
        print(f"\r{done}/{pairs}", end="", flush=True)
    print()
    return out_dir


MASK_NAMES = ("left", "right", "top", "bottom", "center")


def mask_of(spec, shape):
    """``--inpaint MASK`` as a float [H, W] (or [1 | N, 1, H, W] from a file) mask, 1 = keep: a half-image name keeps that half, "center"
    generates the central half-side square; anything else is a tensor file or a picture (grey level / 255)."""
    H, W = shape[1], shape[2]
    if spec in MASK_NAMES:
        m = torch.zeros(H, W)
        if spec == "left":
            m[:, :W // 2] = 1
        elif spec == "right":
            m[:, W - W // 2:] = 1
        elif spec == "top":
            m[:H // 2] = 1
        elif spec == "bottom":
            m[H - H // 2:] = 1
        else:
            m[:] = 1
            m[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 0
        return m
    if not os.path.isfile(spec):
        raise ValueError(f"--inpaint {spec!r}: expected one of {', '.join(MASK_NAMES)} or a mask file")
    if spec.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")):
        import numpy as np
        from PIL import Image
        return torch.from_numpy(np.asarray(Image.open(spec).convert("L")).copy()).float() / 255.0
    m = torch.load(spec, map_location="cpu")
    if not torch.is_tensor(m):
        raise ValueError(f"--inpaint {spec}: expected a tensor, got {type(m).__name__}")
    return m


def condition(args):
    """--inpaint / --edit-start: deterministic file names (inpaint_00000.png, ...), so a seeded run repeats byte for byte."""
    from ddpm_torch.utils import save_image_grid
    process, model, device, shape, out_dir = build(args)
    os.makedirs(out_dir, exist_ok=True)
    src = load_source(args.source, shape)
    mask = mask_of(args.inpaint, shape) if args.inpaint else None
    num_classes = next((m.num_classes for m in model.modules() if getattr(m, "num_classes", None) is not None), None)
    done = chain = 0
    for i in range(0, len(src), args.batch_size):
        x = src[i:i + args.batch_size].to(device)
        y = labels_of(args.labels, num_classes, done, len(x), device) if args.labels else None
        seed = None if args.seed is None else args.seed + chain
        if mask is None:
            out = process.edit(model, x, args.edit_start, seed=seed, y=y)
            panels = [x, out]
        else:
            m = mask[i:i + len(x)] if mask.ndim == 4 and mask.shape[0] > 1 else mask
            out = process.inpaint(model, x, m, jump_length=args.jump_length, resamples=args.resamples, start=args.edit_start, seed=seed, y=y)
            shown = m.to(device).float().reshape((-1, 1) + tuple(shape[1:]))
            panels = [x, x * shown, out]                          # the open region of the masked source is mid-grey
        for j in range(len(x)):
            save_image_grid(torch.stack([p[j] for p in panels]), os.path.join(out_dir, f"inpaint_{done + j:05d}.png"), nrow=len(panels))
        done += len(x)
        chain += 1
        print(f"\r{done}/{len(src)}", end="", flush=True)
    print()
    return out_dir


def main(argv=None):
    args = parse_args(argv)
    if args.inpaint or args.edit_start is not None:
        return condition(args)
    if args.interpolate or args.reconstruct:
        return invert(args)
    if args.num_gpus > 1:
        import torch.multiprocessing as mp
        mp.set_start_method("spawn")
        mp.spawn(generate, args=(args,), nprocs=args.num_gpus)
        return None
    return generate(0, args)


if __name__ == "__main__":
    main()
