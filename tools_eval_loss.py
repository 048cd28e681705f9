#!/usr/bin/env python3
"""Score a checkpoint on held-out structures: the denoising loss per noise level and the trainer's validation loss.

    tools_eval_loss.py --model_path DIR [--model_checkpoint best] --data X.pt|X.npy --levels 0:100:5 [--draws 4] [--loss_type l2]

DIR is a saved_models/<mol>-style directory (args.pickle + model-<checkpoint>.pt) as the sampling CLI reads it; the data
are structures (n, N, 3) in Angstrom, as the trainer's validation loader yields them.  Prints ONE JSON object:
"profile" -- per level the fp64 mean loss over n * draws noised structures (dff_amd.loss_profile) -- and "forward_loss",
Trainer.eval_loss over the same data (levels drawn from the model's p2_loss_weight; the number `best` is chosen by).
Run it once per checkpoint (best, last, 1, 2, 3, ...) to rank them, and read the profile to choose --noise_level."""
import argparse
import json
import sys

import numpy as np
import torch


def parse_levels(text: str):
    """"a:b:c" -> range(a, b, c) (c optional), or a comma-separated list."""
    if ":" in text:
        parts = [int(p) for p in text.split(":")]
        if not 2 <= len(parts) <= 3:
            raise argparse.ArgumentTypeError("--levels takes start:stop[:step] or a comma-separated list")
        return list(range(*parts))
    return [int(p) for p in text.split(",") if p]


def load_structures(path: str) -> torch.Tensor:
    x = torch.from_numpy(np.load(path)) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    x = torch.as_tensor(x, dtype=torch.float32)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"{path}: expected structures of shape (n, N, 3), got {tuple(x.shape)}")
    return x


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--model_path", required=True)
    p.add_argument("--model_checkpoint", default="best", help="best, last, 1, 2, 3, ...")
    p.add_argument("--data", required=True, help="X.pt or X.npy: (n, N, 3) structures in Angstrom")
    p.add_argument("--levels", type=parse_levels, default=parse_levels("0:100:5"))
    p.add_argument("--draws", type=int, default=4, help="independent noisings of every structure per level")
    p.add_argument("--loss_type", default="l2", choices=("l1", "l2"))
    p.add_argument("--batch_size", type=int, default=4096)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=int, default=0)
    a = p.parse_args(argv)

    from dff_amd import cli, losses
    targs = cli.load_training_args(a.model_path)
    ddpm, mol = cli.build_diffusion(targs, a.model_path, a.model_checkpoint, torch.device("cuda", a.device), seed=a.seed)
    ddpm.loss_type = a.loss_type
    data = load_structures(a.data)
    if data.shape[1] != mol.n_beads:
        raise ValueError(f"{a.data} has {data.shape[1]} beads, the model {mol.n_beads}")
    bad = [l for l in a.levels if not 0 <= l < ddpm.num_timesteps]
    if bad:
        raise ValueError(f"levels outside 0 .. {ddpm.num_timesteps - 1}: {bad}")
    prof = losses.loss_profile(ddpm, data, a.levels, draws=a.draws, batch_size=a.batch_size)
    batches = [data[i:i + a.batch_size] for i in range(0, data.shape[0], a.batch_size)]
    fwd = float(losses.eval_loss(ddpm, batches, len(batches)))
    ddpm.model.native.check()
    out = {"model_path": a.model_path, "checkpoint": a.model_checkpoint, "mol": targs.mol, "structures": int(data.shape[0]),
           "loss_type": a.loss_type, "draws": a.draws, "seed": a.seed, "loss_weights": ddpm.loss_weights,
           "profile": [{"level": int(l), "loss": float(v), "count": int(c)}
                       for l, v, c in zip(prof["levels"], prof["loss"], prof["count"])],
           "forward_loss": fwd}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
    sys.exit(0)
