"""
The denoising loss of a fixed checkpoint (forward only): what the reference's ``validation_step`` reports.

Two layers:

* ``radian_smooth_l1_loss`` / ``smooth_l1_loss``: host restatements of foldingdiff/losses.py:29-63 and of
  ``torch.nn.functional.smooth_l1_loss`` with the reference's signatures, the same torch operations in the same order
  (bit-identical to the reference on the same host).  They are the statement of what the device computes and what the
  tests pin to the golden fixture; the product path does not call them.
* ``loss_terms``: the per-position terms and their per-sequence fp64 sums on the device (``fd_loss_terms``,
  csrc/loss.hip).  The model-level entry, which also runs the forward, is ``BertForDiffusionBase.loss_terms``.

Not built (the reference offers them, this package says so instead of approximating): the "l1" loss
(``radian_l1_loss``), the pairwise-distance loss (``pairwise_dist_loss``: a differentiable NeRF + CA pdist) and the circle
penalty (``circle_penalty`` must be 0).
"""
from typing import Sequence, Tuple, Union

import numpy as np
import torch

from . import _binding, utils

ANGULAR_BETA = torch.pi / 10    # modelling.py: angular_loss_fn_dict["smooth_l1"] = partial(radian_smooth_l1_loss, beta=torch.pi / 10)
NONANGULAR_BETA = 1.0           # F.smooth_l1_loss's default


def radian_smooth_l1_loss(input: torch.Tensor, target: torch.Tensor, beta: float = 1.0,
                          circle_penalty: float = 0.0) -> torch.Tensor:
    """
    Smooth L1 loss of the wrapped difference: |d| < beta -> 0.5 d^2 / beta, else |d| - 0.5 beta, mean over all elements.
    >>> radian_smooth_l1_loss(torch.tensor(-17.0466), torch.tensor(-1.3888), beta=0.1)
    tensor(3.0414)
    """
    if circle_penalty != 0:
        raise NotImplementedError("circle_penalty (the reference's circle_reg) is not built; it must be 0")
    input, target = torch.as_tensor(input), torch.as_tensor(target)
    assert target.shape == input.shape, f"Mismatched shapes: {input.shape} != {target.shape}"
    assert beta > 0
    return torch.mean(_radian_terms(input, target, beta))


def _radian_terms(input: torch.Tensor, target: torch.Tensor, beta: float) -> torch.Tensor:
    d = target - input
    d = utils.modulo_with_wrapped_range(d, -torch.pi, torch.pi)
    abs_d = torch.abs(d)
    return torch.where(abs_d < beta, 0.5 * (d**2) / beta, abs_d - 0.5 * beta)


def smooth_l1_loss(input: torch.Tensor, target: torch.Tensor, beta: float = 1.0) -> torch.Tensor:
    """``F.smooth_l1_loss(input, target, beta=beta)`` with the default mean reduction (the non-angular features)."""
    return torch.nn.functional.smooth_l1_loss(torch.as_tensor(input), torch.as_tensor(target), beta=beta)


def host_terms(pred: torch.Tensor, target: torch.Tensor, ft_is_angular: Sequence[bool],
               beta_ang: float = ANGULAR_BETA, beta_lin: float = NONANGULAR_BETA) -> torch.Tensor:
    """Per-position terms [..., F] on the host, feature by feature with the two functions above (no mask applied)."""
    cols = []
    for f, ang in enumerate(ft_is_angular):
        p, t = pred[..., f], target[..., f]
        cols.append(_radian_terms(p, t, beta_ang) if ang
                    else torch.nn.functional.smooth_l1_loss(p, t, beta=beta_lin, reduction="none"))
    return torch.stack(cols, dim=-1)


def lengths_of(lengths_or_mask, L: int) -> np.ndarray:
    """int32 [B] lengths from a [B] vector of lengths or a [B, L] prefix mask (ones, then zeros)."""
    a = lengths_or_mask.detach().cpu().numpy() if isinstance(lengths_or_mask, torch.Tensor) else np.asarray(lengths_or_mask)
    if a.ndim == 1:
        return np.ascontiguousarray(a.astype(np.int32))
    if a.ndim != 2 or a.shape[1] != L:
        raise ValueError(f"expected [B] lengths or a [B, {L}] mask, got shape {a.shape}")
    on = a != 0
    lens = on.sum(axis=1)
    if not np.array_equal(on, np.arange(L)[None, :] < lens[:, None]):
        raise ValueError("the mask is not a prefix mask (ones followed by zeros)")
    return np.ascontiguousarray(lens.astype(np.int32))


def loss_terms(pred, target, lengths_or_mask, ft_is_angular: Sequence[bool], device: int = 0,
               beta_ang: float = ANGULAR_BETA, beta_lin: float = NONANGULAR_BETA,
               return_terms: bool = True) -> Union[np.ndarray, Tuple[np.ndarray, np.ndarray]]:
    """The smooth-L1 terms of ``pred`` against ``target`` ([B, L, F] float32) on the device.  Returns ``(sums, terms)``:
    ``sums`` float64 [B, F], the terms of sequence b summed over its first ``lengths[b]`` positions (fixed order: the
    same bits from run to run and wherever the sequence sits in the batch), and ``terms`` float32 [B, L, F] with zeros at
    masked positions (``return_terms=False``: ``sums`` alone).  ``_get_loss_terms``' value of feature f is
    ``sums[:, f].sum() / lengths.sum()``."""
    as_np = lambda v: np.ascontiguousarray((v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float32, copy=False))  # noqa: E731
    p, t = as_np(pred), as_np(target)
    if p.ndim != 3 or p.shape != t.shape:
        raise ValueError(f"pred {p.shape} and target {t.shape} must be the same [B, L, F]")
    B, L, F = p.shape
    if len(ft_is_angular) != F:
        raise ValueError(f"{len(ft_is_angular)} angular flags for {F} features")
    lens = lengths_of(lengths_or_mask, L)
    if lens.shape != (B,):
        raise ValueError(f"{lens.shape[0]} lengths for a batch of {B}")
    flags = np.ascontiguousarray(np.asarray(ft_is_angular, dtype=np.uint8))
    sums = np.empty((B, F), np.float64)
    terms = np.empty((B, L, F), np.float32) if return_terms else None
    _binding.check(_binding.load().fd_loss_terms(int(device), _binding.ptr(p), _binding.ptr(t), _binding.ptr(lens), B, L, F,
                                                 _binding.ptr(flags), float(beta_ang), float(beta_lin), _binding.ptr(sums),
                                                 _binding.ptr(terms)))
    return (sums, terms) if return_terms else sums
