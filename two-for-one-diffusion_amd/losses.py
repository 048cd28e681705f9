"""Scoring a model on held-out structures: the validation loss of the reference's trainer and the loss as a function
of the noise level.

``eval_loss`` is ``Trainer.eval_loss`` (trainer.py:222-235) -- the number the trainer ranks checkpoints by (``best``).
``loss_profile`` is the same loss at fixed noise levels: where it is small the network denoises well, which is what
``--noise_level`` needs of a force field.  Both go through ``GaussianDiffusion.p_losses`` (one ``dff_denoise_loss`` call per batch).
"""
from __future__ import annotations

import numpy as np
import torch

from .ddpm import center_zero


@torch.no_grad()
def eval_loss(ddpm, batches, val_iters: int, t_diff_range=None):
    """trainer.py:222-235: the mean over ``val_iters`` batches of ``ddpm(batch)``.  ``batches`` yields tensors
    (B, N, 3) in Angstrom, or tuples whose first entry is one (a DataLoader over a TensorDataset).  0-d tensor."""
    it = iter(batches)
    loss = 0
    for _ in range(val_iters):
        batch = next(it)
        if isinstance(batch, (list, tuple)):
            batch = batch[0]
        loss = loss + ddpm(batch.to(ddpm.device), t_diff_range=t_diff_range).mean()
    return loss / val_iters


@torch.no_grad()
def loss_profile(ddpm, data, levels, draws: int = 1, batch_size: int = 4096):
    """The denoising loss of ``data`` (n, N, 3; Angstrom: centred and divided by norm_factor here, as ``forward`` does) at
    each noise level of ``levels``, every structure noised ``draws`` times: a dict of ``levels`` (int64), ``loss`` (float64:
    the mean of the per-sample losses, summed in fp64 on the device) and ``count`` (int64: n * draws).
    Structure i, draw d is keyed (seed; item i, step FORWARD_STEP | d) whatever the batch size, and the same key is used at
    every level (common random numbers: the profile is smooth in the level).  The sums stay on the device; the host reads
    them once, at the end."""
    levels = [int(l) for l in levels]
    x = center_zero(data.detach().to(ddpm.device, torch.float32)) / ddpm.norm_factor
    n = x.shape[0]
    totals = torch.zeros((len(levels), 2), dtype=torch.float64, device=ddpm.device)
    for lo in range(0, n, batch_size):
        xb = x[lo:lo + batch_size].contiguous()
        for k, level in enumerate(levels):
            t = torch.full((xb.shape[0],), level, dtype=torch.int32, device=ddpm.device)
            for d in range(draws):
                ddpm.p_losses(xb, t, sample_offset=lo, draw=d, total=totals[k])
    tot = totals.cpu().numpy()
    count = tot[:, 1].astype(np.int64)
    return {"levels": np.asarray(levels, np.int64), "loss": tot[:, 0] / np.maximum(count, 1), "count": count}
