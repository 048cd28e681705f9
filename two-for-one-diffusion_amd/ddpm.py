"""Host mirror of ``GaussianDiffusion`` (models/ddpm.py:20-337): the sampling half and the forward process with its loss.

The reverse loop itself -- 1000 score-network calls, each followed by the posterior update,
the +-1000 clamp and the centring -- runs inside ONE persistent HIP kernel launch
(``dff_ddpm_run``); nothing syncs with the host per step (the reference syncs three times per
step: utils.py:79, ddpm.py:248).
"""
from __future__ import annotations

import math
import warnings
from typing import Optional

import torch

from . import binding
from .score import GraphTransformer


def extract(a, t, x_shape):
    """utils.py:33-39."""
    b, *_ = t.shape
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))


def center_zero(x):
    """utils.py:65-70."""
    assert len(x.shape) == 3 and x.shape[-1] == 3, "Dimensionality error"
    return x - x.mean(dim=1, keepdim=True)


def assert_center_zero(x, eps=1e-3):
    """utils.py:73-86 (one host sync; used only at the very end of a chain)."""
    assert len(x.shape) == 3 and x.shape[-1] == 3, "Dimensionality error"
    center_max = x.mean(dim=1).abs().max().item()
    if center_max >= eps:
        raise AssertionError(f"Center not at zero: abs max at {center_max}")


def _cosine_schedule64(timesteps: int, s: float = 0.008):
    """(betas, alphas_cumprod) of the cosine schedule in float64, operation by operation as utils.py:52-62 and
    ddpm.py:52-53 compute them: the loss-weight tables are functions of these, not of their float32 roundings."""
    x = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64)
    ac = torch.cos(((x / timesteps) + s) / (1 + s) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    betas = torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)
    return betas, torch.cumprod(1.0 - betas, dim=0)


def p2_loss_weight_table(loss_weights="ones", timesteps: int = 1000, p2_loss_weight_gamma: float = 0.0,
                         p2_loss_weight_k: float = 1):
    """The float32 ``p2_loss_weight`` buffer of ddpm.py:100-138 (CPU tensor): the distribution ``forward`` draws the
    noise levels from.  Branch order, parsing and the exception are the reference's."""
    betas, ac = _cosine_schedule64(timesteps)
    if loss_weights == "ones":
        w = (p2_loss_weight_k + ac / (1 - ac)) ** -p2_loss_weight_gamma
    elif loss_weights == "score_matching":
        w = 1.0 / (1 - ac)                      # (the reference registers the unnormalised weights)
    elif "higheruntil_" in loss_weights:
        threshold = int(loss_weights.split("_")[1])
        w = torch.Tensor([len(ac) / threshold] * threshold + [len(ac) / (len(ac) - threshold)] * (len(ac) - threshold))
    elif "lower_bound" in loss_weights:
        clamp_val = int(loss_weights.split("_")[2])
        unnormalized = (1.0 / ((1 - ac) * (1 - betas))).clip(0, clamp_val)
        w = unnormalized / sum(unnormalized) * len(betas)   # (Python's sum: element by element, as the reference adds)
    else:
        raise Exception(f"Wrong loss_weights: {loss_weights}")
    return w.to(torch.float32)


def p2_loss_weight_tables(requests):
    """[p2_loss_weight_table(*r) for r in requests] as numpy arrays (one call for several tables)."""
    return [p2_loss_weight_table(*r).numpy() for r in requests]


class GaussianDiffusion:
    def __init__(self, model: GraphTransformer, features=None, num_atoms: Optional[int] = None,
                 timesteps: int = 1000, loss_type="l2", objective="pred_noise", beta_schedule="cosine",
                 p2_loss_weight_gamma: float = 0.0, p2_loss_weight_k: float = 1,
                 norm_factor: float = 1, loss_weights="ones", seed: int = 0,
                 defer_checks: bool = False):
        if objective != "pred_noise" or beta_schedule != "cosine":
            raise ValueError("only objective='pred_noise', beta_schedule='cosine' (the shipped configs) are supported")
        self.dims = 3
        self.model = model
        self.num_atoms = model.num_beads if num_atoms is None else num_atoms
        self.device = model.device
        self.h = torch.eye(self.num_atoms, device=self.device) if features is None else features.to(self.device)
        self.objective = objective
        self.num_timesteps = int(timesteps)
        if model.native.timesteps != self.num_timesteps:
            raise ValueError("model was built for a different number of diffusion steps")
        self.norm_factor = norm_factor
        self.loss_weights = loss_weights
        self.loss_type = loss_type
        self.p2_loss_weight = p2_loss_weight_table(loss_weights, self.num_timesteps, p2_loss_weight_gamma,
                                                   p2_loss_weight_k).to(self.device)
        for name in binding.SCHEDULE_NAMES:  # the 12 float32 buffers of ddpm.py:61-99
            setattr(self, name, torch.from_numpy(model.native.schedule(name)).to(self.device))
        self._seed = int(seed)
        self._samples_drawn = 0
        self._noised = 0   # structures noised so far by q_sample / p_losses with in-kernel draws: their Philox item offset
        self.last_clamped = False
        # ONE device flag word for the lifetime of the object, handed to every fused launch and never reset by the
        # kernels: bit 0 = the +-1000 clamp fired somewhere (ddpm.py:248-250 warns per step), bit 1 = a chain ended with
        # a centre of mass >= 1e-3 (assert_center_zero, ddpm.py:252).  check_clamp() reads and clears it.
        self._flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        # The reference warns about the clamp per step and asserts a centred result at the end of every p_sample_loop
        # (ddpm.py:248-252).  Here every chain entry point (sample, p_sample_loop, p_sample_loop_from) ends with ONE
        # check_clamp() -- one host sync per chain instead of three per step -- so a library user gets the warning and the
        # assertion without having to remember anything.  defer_checks=True leaves the word alone until the caller's own
        # check_clamp() (the CLI and bench.py run many batches back to back and check once at the end).
        self.defer_checks = bool(defer_checks)

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def seed(self, seed: int):
        self._seed, self._samples_drawn, self._noised = int(seed), 0, 0

    @torch.no_grad()
    def p_mean_variance(self, x, t):
        """ddpm.py:195-219 with the score network on the HIP path (``dff_score``)."""
        assert_center_zero(x)                                                   # ddpm.py:199
        model_output = center_zero(self.model(x, self.h, 1.0 * t / self.num_timesteps))
        x_start = (extract(self.sqrt_recip_alphas_cumprod, t, x.shape) * x
                   - extract(self.sqrt_recipm1_alphas_cumprod, t, x.shape) * model_output)
        x_start = center_zero(x_start)
        mean = (extract(self.posterior_mean_coef1, t, x.shape) * x_start
                + extract(self.posterior_mean_coef2, t, x.shape) * x)
        return (mean, extract(self.posterior_variance, t, x.shape),
                extract(self.posterior_log_variance_clipped, t, x.shape))

    @torch.no_grad()
    def p_sample(self, x, t, noise=None):
        """One reverse step for arbitrary per-sample ``t`` (ddpm.py:221-232): score op on the
        HIP kernel, the O(N) posterior arithmetic as device tensor ops.  The sampler proper does
        not come through here -- ``p_sample_loop`` runs all steps fused in one launch."""
        x = x.detach().to(self.device, torch.float32).contiguous()
        t = t.to(self.device)
        b = x.shape[0]
        mean, _, logvar = self.p_mean_variance(x, t)
        noise = torch.randn_like(x) if noise is None else noise.to(self.device, torch.float32)
        noise = center_zero(noise)
        nonzero_mask = (1 - (t == 0).float()).reshape(b, *((1,) * (len(x.shape) - 1)))
        return mean + nonzero_mask * (0.5 * logvar).exp() * noise

    @torch.no_grad()
    def p_sample_loop_from(self, x, t_start: int, t_end: int = 0, noises=None):
        """Reverse steps t_start..t_end from a given centred x, each followed by the clamp and
        centring of p_sample_loop (ddpm.py:244-251); normalised units in and out."""
        x = x.detach().to(self.device, torch.float32).contiguous().clone()
        # the reference's p_mean_variance asserts a centred input at every step (ddpm.py:195-199 via utils.py:73-86); the
        # fused loop uses x as it comes, so an un-centred start would silently diverge from the reference: refuse it here
        assert_center_zero(x)
        if noises is not None:
            noises = noises.detach().to(self.device, torch.float32).contiguous()
        self.model.native.ddpm_run(x, t_start, t_end, noise=noises, seed=self._seed,
                                   sample_offset=self._samples_drawn, clamp_flag=self._flag)
        if not self.defer_checks:
            self.check_clamp()
        return x

    @torch.no_grad()
    def p_sample_loop(self, shape):
        """ddpm.py:234-254: x_T = center_zero(randn) then T reverse steps, all on the device."""
        b = shape[0]
        x = torch.empty(shape, device=self.device, dtype=torch.float32)
        self.model.native.ddpm_run(x, self.num_timesteps - 1, 0, noise=None, seed=self._seed,
                                   sample_offset=self._samples_drawn, init_prior=True, clamp_flag=self._flag)
        self._samples_drawn += b
        if not self.defer_checks:
            self.check_clamp()                                                   # ddpm.py:249,252
        return x

    def check_clamp(self) -> bool:
        """ONE host read of the device flag word for everything launched since the last call (the reference syncs three
        times per step): warns like ddpm.py:249 if the clamp fired in ANY batch, raises like assert_center_zero
        (ddpm.py:252) if any chain ended off-centre; clears the word."""
        word = int(self._flag.item())
        self.last_clamped = bool(word & 1)
        self._flag.zero_()
        try:
            self.model.native.check()   # (the read above synchronised the device)
        except RuntimeError:
            # the chains since the last check are invalid, but what their flag word said is not lost with the exception
            if self.last_clamped:
                warnings.warn("Large molecule encountered in sampling")
            raise
        if self.last_clamped:
            warnings.warn("Large molecule encountered in sampling")
        if word & 2:
            raise AssertionError("Center not at zero: a reverse chain ended with |centre of mass| >= 0.001")
        return self.last_clamped

    @torch.no_grad()
    def sample(self, batch_size):
        """ddpm.py:256-263: (batch_size, N, 3) in Angstrom (x norm_factor), device tensor."""
        return self.p_sample_loop((batch_size, self.num_atoms, self.dims)) * self.norm_factor

    # ---- the forward process and its loss (ddpm.py:164-193, 265-337)
    @torch.no_grad()
    def q_mean_variance(self, x_start, t):
        """ddpm.py:163-171."""
        mean = extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        variance = extract(1.0 - self.alphas_cumprod, t, x_start.shape)
        log_variance = extract(self.log_one_minus_alphas_cumprod, t, x_start.shape)
        return mean, variance, log_variance

    @torch.no_grad()
    def assert_normal_kl(self, x_start, t, eps=1e-4):
        """ddpm.py:173-193: KL(q(x_T | x_0) || N(0, 1)) must be close to zero (enough diffusion steps for data of this
        scale).  One host read."""
        assert_center_zero(x_start)
        mean1, _, logvar1 = self.q_mean_variance(x_start, t)
        logvar1 = logvar1.squeeze()
        mean2, logvar2 = torch.zeros_like(mean1), torch.zeros_like(logvar1)
        meandifsq = ((mean1 - mean2) ** 2).sum(dim=(-2, -1))
        normal_kl = 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2) + meandifsq * torch.exp(-logvar2))
        kl = normal_kl.abs().max().item()
        assert kl <= eps, f"Normal KL check at T failed, max value: {kl}"

    def _forward_inputs(self, x_start, t, noise, sample_offset):
        x_start = x_start.detach().to(self.device, torch.float32).contiguous()
        t = torch.as_tensor(t).to(self.device)
        if noise is not None:
            noise = noise.detach().to(self.device, torch.float32).contiguous()
        elif sample_offset is None:      # in-kernel draws: this call's structures take the next items of the object's stream
            sample_offset = self._noised
            self._noised += x_start.shape[0]
        return x_start, t, noise, sample_offset or 0

    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None, sample_offset=None, draw: int = 0):
        """ddpm.py:265-274 followed by the centring of p_losses (:296), on the device (``dff_q_sample``).  Without
        ``noise`` the draws come from the object's Philox stream (``seed``): every call advances a counter by its batch, so
        two calls never share noise; ``sample_offset`` / ``draw`` name the items explicitly instead (no counter)."""
        x_start, t, noise, off = self._forward_inputs(x_start, t, noise, sample_offset)
        return self.model.native.q_sample(x_start, t, noise=noise, seed=self._seed, sample_offset=off, draw=draw)

    @torch.no_grad()
    def p_losses(self, x_start, t, noise=None, sample_offset=None, draw: int = 0, total=None):
        """ddpm.py:288-315 for objective "pred_noise": the mean over the batch of the per-sample l1 / l2 loss, a 0-d
        tensor.  Diffusion, score and loss are one library call (``dff_denoise_loss``); noise as in ``q_sample``.
        ``total`` (float64 CUDA tensor of 2) accumulates (sum of the per-sample losses, batch) on the device."""
        if self.loss_type not in binding.LOSS_TYPES:
            raise ValueError(f"invalid loss type {self.loss_type}")
        x_start, t, noise, off = self._forward_inputs(x_start, t, noise, sample_offset)
        loss = self.model.native.denoise_loss(x_start, t, noise=noise, seed=self._seed, sample_offset=off, draw=draw,
                                              loss_type=self.loss_type, total=total)
        return loss.mean()

    @torch.no_grad()
    def forward(self, mol, *args, t_diff_range=None, **kwargs):
        """ddpm.py:317-337: centre ``mol`` (Angstrom), divide by norm_factor, draw one noise level per structure from
        ``p2_loss_weight``, check the KL to the prior at T - 1, return ``p_losses``.  ``t_diff_range`` is accepted and
        unused, exactly as in the reference (ddpm.py:317: the trainer passes it, nothing reads it)."""
        mol = center_zero(mol.detach().to(self.device, torch.float32)) / self.norm_factor
        assert_center_zero(mol)
        b, n, d = mol.shape
        assert n == self.num_atoms and d == self.dims, f"Molecule shape must be {(self.num_atoms, self.dims)}"
        t = torch.multinomial(self.p2_loss_weight, b, replacement=True).long()
        self.assert_normal_kl(x_start=mol, t=torch.full((b,), self.num_timesteps - 1, device=self.device, dtype=torch.long))
        return self.p_losses(mol, t, *args, **kwargs)

    __call__ = forward
