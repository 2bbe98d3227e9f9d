"""
The denoising loss of a fixed checkpoint (forward only): what the reference's ``validation_step`` reports, for every
setting ``BertForDiffusion`` can be trained with -- ``loss`` "smooth_l1" or "l1", the circle penalty (``circle_reg``)
and the pairwise-distance term (``use_pdist_loss``).

Two layers:

* host restatements of foldingdiff/losses.py and of the statements of ``_get_loss_terms`` around them
  (modelling.py:616-677), with the reference's signatures and the same torch operations in the same order
  (bit-identical to the reference on the same host): ``radian_smooth_l1_loss`` / ``smooth_l1_loss`` /
  ``radian_l1_loss`` / ``circle_turns`` / ``denoised_angles`` / ``pairwise_coef`` / ``pairwise_dist_loss``, and
  ``pairwise_dist_host``, an fp64 numpy statement of what the pairwise kernel computes.  They are the statement of
  what the device computes and what the tests pin to the golden fixtures; the product path does not call them.
* ``loss_terms`` and ``pairwise_dist_sums``: the per-position terms, the turn counts and the pair terms with their
  per-sequence fp64 sums on the device (``fd_loss_terms``, ``fd_loss_terms_ex``, ``fd_pairwise_dist``; csrc/loss.hip,
  csrc/loss_variants.hip).  The model-level entry, which also runs the forward, is ``BertForDiffusionBase.loss_terms``.

``radian_smooth_l1_loss`` itself still refuses ``circle_penalty != 0``, as it always has here; the penalised value
is ``radian_smooth_l1_circle_loss``.

Not built: mixed timesteps with arbitrary (non-prefix) masks, and sharding a batch across ranks.
"""
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _binding, utils

LOSS_KINDS = {"smooth_l1": 0, "l1": 1}         # fd_loss_terms_ex's kind
LOSS_AUTOCORRECT = {"radian_l1_smooth": "smooth_l1"}   # modelling.py: loss_autocorrect_dict (legacy checkpoints)
PAIRWISE_ANGLES = ("phi", "psi", "omega", "tau", "CA:C:1N", "C:1N:1CA")   # what nerf_build_batch is given, in feat_idx order
PAIRWISE_MAX_LEN = 128
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
        raise NotImplementedError("circle_penalty must be 0 here: radian_smooth_l1_circle_loss is the penalised value")
    input, target = torch.as_tensor(input), torch.as_tensor(target)
    assert target.shape == input.shape, f"Mismatched shapes: {input.shape} != {target.shape}"
    assert beta > 0
    return torch.mean(_radian_terms(input, target, beta))


def _radian_terms(input: torch.Tensor, target: torch.Tensor, beta: float) -> torch.Tensor:
    d = target - input
    d = utils.modulo_with_wrapped_range(d, -torch.pi, torch.pi)
    abs_d = torch.abs(d)
    return torch.where(abs_d < beta, 0.5 * (d**2) / beta, abs_d - 0.5 * beta)


def circle_turns(input: torch.Tensor) -> torch.Tensor:
    """``torch.div(torch.abs(input), torch.pi, rounding_mode="trunc")``: the whole turns of pi in |input| (losses.py:59-61)."""
    return torch.div(torch.abs(torch.as_tensor(input)), torch.pi, rounding_mode="trunc")


def radian_smooth_l1_circle_loss(input: torch.Tensor, target: torch.Tensor, beta: float = 1.0,
                                 circle_penalty: float = 0.0) -> torch.Tensor:
    """The reference's ``radian_smooth_l1_loss`` in full (losses.py:29-63): the mean smooth-L1 term of the wrapped
    difference, plus ``circle_penalty * mean(trunc(|input| / pi))`` when ``circle_penalty > 0`` (``input`` is the
    predicted noise)."""
    input, target = torch.as_tensor(input), torch.as_tensor(target)
    retval = radian_smooth_l1_loss(input, target, beta=beta)
    if circle_penalty > 0:
        retval += circle_penalty * torch.mean(circle_turns(input))
    return retval


def radian_l1_loss(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """
    Mean absolute angular difference (losses.py:12-26); takes no circle penalty.
    >>> radian_l1_loss(torch.tensor(0.1), torch.tensor(2 * torch.pi - 0.1))
    tensor(0.2000)
    """
    return torch.mean(_radian_l1_terms(torch.as_tensor(input), torch.as_tensor(target)))


def _radian_l1_terms(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    target = target % (2 * torch.pi)
    input = input % (2 * torch.pi)
    d = target - input
    d = (d + torch.pi) % (2 * torch.pi) - torch.pi
    return torch.abs(d)


def smooth_l1_loss(input: torch.Tensor, target: torch.Tensor, beta: float = 1.0) -> torch.Tensor:
    """``F.smooth_l1_loss(input, target, beta=beta)`` with the default mean reduction (the non-angular features)."""
    return torch.nn.functional.smooth_l1_loss(torch.as_tensor(input), torch.as_tensor(target), beta=beta)


def host_terms(pred: torch.Tensor, target: torch.Tensor, ft_is_angular: Sequence[bool],
               beta_ang: float = ANGULAR_BETA, beta_lin: float = NONANGULAR_BETA, loss: str = "smooth_l1") -> torch.Tensor:
    """Per-position terms [..., F] on the host, feature by feature with the functions above (no mask applied)."""
    cols = []
    for f, ang in enumerate(ft_is_angular):
        p, t = pred[..., f], target[..., f]
        if LOSS_KINDS[loss] == 1:
            cols.append(_radian_l1_terms(p, t) if ang else torch.nn.functional.l1_loss(p, t, reduction="none"))
            continue
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
               return_terms: bool = True, kind: Union[int, str] = 0,
               return_turns: bool = False) -> Union[np.ndarray, Tuple[np.ndarray, ...]]:
    """The smooth-L1 terms of ``pred`` against ``target`` ([B, L, F] float32) on the device.  Returns ``(sums, terms)``:
    ``sums`` float64 [B, F], the terms of sequence b summed over its first ``lengths[b]`` positions (fixed order: the
    same bits from run to run and wherever the sequence sits in the batch), and ``terms`` float32 [B, L, F] with zeros at
    masked positions (``return_terms=False``: ``sums`` alone).  ``_get_loss_terms``' value of feature f is
    ``sums[:, f].sum() / lengths.sum()``.

    ``kind`` 1 / "l1": the terms of ``radian_l1_loss`` / ``F.l1_loss`` instead (``fd_loss_terms_ex``).
    ``return_turns=True`` appends ``turns`` int64 [B, F] to what is returned: per sequence the sum over its unmasked
    positions of ``circle_turns(pred)`` for angular features, 0 for the others; the circle penalty adds
    ``circle_penalty * turns[:, f].sum() / lengths.sum()`` to feature f's value."""
    kind = LOSS_KINDS[kind] if isinstance(kind, str) else int(kind)
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
    if kind == 0 and not return_turns:
        _binding.check(_binding.load().fd_loss_terms(int(device), _binding.ptr(p), _binding.ptr(t), _binding.ptr(lens), B, L, F,
                                                     _binding.ptr(flags), float(beta_ang), float(beta_lin), _binding.ptr(sums),
                                                     _binding.ptr(terms)))
        return (sums, terms) if return_terms else sums
    turns = np.empty((B, F), np.int64) if return_turns else None
    _binding.check(_binding.load().fd_loss_terms_ex(int(device), _binding.ptr(p), _binding.ptr(t), _binding.ptr(lens), B, L, F,
                                                    _binding.ptr(flags), kind, float(beta_ang), float(beta_lin),
                                                    _binding.ptr(sums), _binding.ptr(terms), _binding.ptr(turns)))
    out = tuple(v for v in (sums, terms, turns) if v is not None)
    return out if len(out) > 1 else sums


# ------------------------------------------------------------------ the pairwise-distance term
def pairwise_columns(ft_names: Sequence[str]) -> np.ndarray:
    """int32 [6]: the columns of phi, psi, omega, tau, CA:C:1N and C:1N:1CA in ``ft_names`` -- all six are needed (the
    reference's ``self.ft_names.index(...)``); a missing one is named."""
    names = list(ft_names)
    missing = [n for n in PAIRWISE_ANGLES if n not in names]
    if missing:
        raise ValueError(f"the pairwise-distance loss needs the six angles {list(PAIRWISE_ANGLES)}; "
                         f"the feature set {names} lacks {missing}")
    return np.ascontiguousarray(np.array([names.index(n) for n in PAIRWISE_ANGLES], np.int32))


def pairwise_is_on(use_pairwise_dist_loss) -> bool:
    """The reference's condition (modelling.py:616-619): a (min, max, timesteps) tuple, or a scalar > 0."""
    return isinstance(use_pairwise_dist_loss, (list, tuple)) or use_pairwise_dist_loss > 0


def denoised_angles(corrupted: torch.Tensor, predicted_noise: torch.Tensor, sqrt_alphas_cumprod_t: torch.Tensor,
                    sqrt_one_minus_alphas_cumprod_t: torch.Tensor) -> torch.Tensor:
    """The predicted x_0 (modelling.py:621-629): ``(corrupted - spread_b * pred) / keep_b`` in float32 in that order;
    not wrapped."""
    bs = sqrt_one_minus_alphas_cumprod_t.shape[0]
    denoised = corrupted - sqrt_one_minus_alphas_cumprod_t.view(bs, 1, 1) * predicted_noise
    denoised /= sqrt_alphas_cumprod_t.view(bs, 1, 1)
    return denoised


def pairwise_coef(use_pairwise_dist_loss, t: torch.Tensor) -> torch.Tensor:
    """The weight of each sequence's pairs (modelling.py:657-669), float32.  Tuple form ``(min_coef, max_coef,
    max_timesteps)``: ``min + (max - min) * ((max_t - t) / max_t)``, the shape of ``t`` ([B, 1] in a collated batch).
    Scalar form: the reference's caller hands ``pairwise_dist_loss`` a python float and crashes on ``weights.ndim``; what
    the code plainly intends is ``loss *= coef``, so the scalar becomes a 0-dim float32 tensor, which takes that branch."""
    if isinstance(use_pairwise_dist_loss, (list, tuple)):
        min_coef, max_coef, max_timesteps = use_pairwise_dist_loss
        assert 0 < min_coef < max_coef
        coef = min_coef + (max_coef - min_coef) * ((max_timesteps - t) / max_timesteps)
        assert torch.all(coef > 0)
        return coef
    assert use_pairwise_dist_loss > 0
    return torch.tensor(float(use_pairwise_dist_loss), dtype=torch.float32)


def _get_pairwise_dist_batch(values: torch.Tensor, lengths) -> Tuple[torch.Tensor, torch.Tensor]:
    assert values.ndim == 3 and values.shape[-1] == 3, f"Expected 3D tensor of (batch, N, 3), got {values.shape}"
    assert lengths.ndim == 1 and values.shape[0] == lengths.shape[0]
    dists = [torch.nn.functional.pdist(values[i, :l]) for i, l in enumerate(lengths)]
    max_len = max(len(v) for v in dists)
    mask = torch.zeros((len(dists), max_len))
    retval = torch.zeros((len(dists), max_len))   # float32: the float64 distances are rounded on the way in
    for i, v in enumerate(dists):
        mask[i, :len(v)] = 1.0
        retval[i, :len(v)] = v
    return retval, mask


def pairwise_dist_loss(input: torch.Tensor, target: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                       weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """losses.py:101-149: the mean over all pairs of the batch of the (weighted) squared difference of the pairwise
    distances of ``input`` and ``target`` ([B, N, 3]; sequence b's first ``lengths[b]`` points).  ``weights`` [B, 1]
    weighs sequence b's pairs; a 0-dim or 1-dim tensor multiplies every pair.  No pairs: NaN."""
    if lengths is None:
        lengths = torch.IntTensor([torch.all(~torch.isnan(input[i]), dim=1).sum() for i in range(input.shape[0])])
    assert lengths.shape[0] == input.shape[0]
    input_dists, input_mask = _get_pairwise_dist_batch(input, lengths)
    target_dists, target_mask = _get_pairwise_dist_batch(target, lengths)
    assert torch.allclose(input_mask, target_mask)
    batch_indices, _seq_indices = torch.where(input_mask)
    loss = torch.nn.functional.mse_loss(input_dists[torch.where(input_mask)], target_dists[torch.where(target_mask)],
                                        reduction="none")
    if weights is not None:
        if weights.ndim > 1:
            assert weights.shape[0] == input.shape[0]
            loss *= weights[batch_indices].squeeze()
        else:
            loss *= weights
    return torch.mean(loss)


def _f32_trig(v: np.ndarray):
    """float32 cos, sin correctly rounded from the float64 result -- what the kernels compute (torch's vectorised float32
    sin / cos may differ from it in the last bit)."""
    v64 = v.astype(np.float64)
    return np.cos(v64).astype(np.float32), np.sin(v64).astype(np.float32)


def _place_host(a, b, c, angle: np.ndarray, length: float, torsion: np.ndarray) -> np.ndarray:
    """nerf.place_dihedral for a batch ([B, 3] float64 atoms, [B] float32 angles): the local displacement in float32,
    the frame in float64."""
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)   # noqa: E731
    bc = unit(c - b)
    n = unit(np.cross(b - a, bc))
    nbc = np.cross(n, bc)
    bl = np.float32(length)
    ca, sa = _f32_trig(angle)
    ct, st = _f32_trig(torsion)
    d = np.stack([-bl * ca, bl * ct * sa, bl * st * sa], axis=-1)
    assert d.dtype == np.float32
    d = d.astype(np.float64)
    return bc * d[:, 0:1] + nbc * d[:, 1:2] + n * d[:, 2:3] + c


def nerf_ca_host(angles: np.ndarray, cols: Sequence[int]) -> np.ndarray:
    """float64 [B, L, 3]: the CA trace of ``nerf.nerf_build_batch`` (nerf.py:207-292) on the columns ``cols`` (phi, psi,
    omega, tau, CA:C:1N, C:1N:1CA) of float32 ``angles`` [B, L, F], every position of the padded length."""
    angles = np.asarray(angles, np.float32)
    B, L = angles.shape[:2]
    phi, psi, omega, tau, a_cacn, a_cnca = (angles[:, :, c] for c in cols)
    seed = np.array([[17.047, 14.099, 3.625], [16.967, 12.784, 4.338], [15.685, 12.755, 5.133]])   # nerf.py:22-24
    p0, p1, p2 = (np.repeat(seed[i][None, :], B, axis=0) for i in range(3))
    out = np.zeros((B, L, 3), np.float64)
    out[:, 0] = p1
    for i in range(L - 1):
        n = _place_host(p0, p1, p2, a_cacn[:, i], 1.34, psi[:, i])
        ca = _place_host(p1, p2, n, a_cnca[:, i], 1.46, omega[:, i])
        c = _place_host(p2, n, ca, tau[:, i], 1.54, phi[:, i + 1])
        out[:, i + 1] = ca
        p0, p1, p2 = n, ca, c
    return out


def pairwise_dist_host(angles, corrupted, pred, keep, spread, lengths, cols: Sequence[int], coef=None):
    """What ``fd_pairwise_dist`` computes, in numpy on the host: ``(sums float64 [B], pairs int64 [B], ca float64
    [B, 2, L, 3])``.  float32 denoised angles and trigonometry, float64 frames, float32 distances and terms, fp64 sums."""
    f32 = lambda v: np.asarray(v, np.float32)   # noqa: E731
    angles, corrupted, pred, keep, spread = f32(angles), f32(corrupted), f32(pred), f32(keep).reshape(-1), f32(spread).reshape(-1)
    B, L = angles.shape[:2]
    den = (corrupted - spread[:, None, None] * pred) / keep[:, None, None]
    assert den.dtype == np.float32
    ca = np.stack([nerf_ca_host(angles, cols), nerf_ca_host(den, cols)], axis=1)
    w = np.ones(B, np.float32) if coef is None else np.broadcast_to(f32(coef).reshape(-1), (B,))
    sums, pairs = np.zeros(B, np.float64), np.zeros(B, np.int64)
    for b, n in enumerate(np.asarray(lengths).reshape(-1)):
        i, j = np.triu_indices(int(n), k=1)
        d = [np.sqrt(((ca[b, c, i] - ca[b, c, j]) ** 2).sum(axis=-1)).astype(np.float32) for c in (0, 1)]
        diff = d[1] - d[0]
        sums[b], pairs[b] = (w[b] * (diff * diff)).astype(np.float64).sum(), len(i)
        ca[b, :, int(n):] = 0.0
    return sums, pairs, ca


def pairwise_dist_sums(angles, corrupted, pred, keep, spread, lengths_or_mask, feat_idx: Sequence[int], coef=None,
                       device: int = 0, return_ca: bool = False):
    """The pairwise-distance term on the device (``fd_pairwise_dist``): ``(sums, pairs)``, float64 / int64 [B] -- per
    sequence the fp64 sum over its ``len (len - 1) / 2`` CA pairs of ``coef[b] * (d_denoised - d_clean)^2`` and the number
    of pairs; the reference's value is ``sums.sum() / pairs.sum()`` (NaN without pairs).  ``angles`` / ``corrupted`` /
    ``pred``: [B, L, F] float32, L <= 128; ``keep`` / ``spread``: [B]; ``feat_idx``: ``pairwise_columns(ft_names)``;
    ``coef``: None (1), a scalar, or one weight per sequence.  ``return_ca=True`` appends the float64 [B, 2, L, 3] CA
    traces of the clean and of the denoised angles."""
    as_np = lambda v: np.ascontiguousarray((v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float32, copy=False))  # noqa: E731
    a, c, p = as_np(angles), as_np(corrupted), as_np(pred)
    if a.ndim != 3 or a.shape != c.shape or a.shape != p.shape:
        raise ValueError(f"angles {a.shape}, corrupted {c.shape} and pred {p.shape} must be the same [B, L, F]")
    B, L, F = a.shape
    k, s = as_np(keep).reshape(-1), as_np(spread).reshape(-1)
    if k.shape != (B,) or s.shape != (B,):
        raise ValueError(f"keep / spread must hold one value per sequence ({B})")
    w = None
    if coef is not None:
        w = as_np(coef).reshape(-1)
        w = np.ascontiguousarray(np.broadcast_to(w, (B,))) if w.size == 1 else w
        if w.shape != (B,):
            raise ValueError(f"coef must be a scalar or hold one value per sequence ({B})")
    idx = np.ascontiguousarray(np.asarray(feat_idx, np.int32).reshape(-1))
    if idx.shape != (6,):
        raise ValueError("feat_idx holds the six columns of phi, psi, omega, tau, CA:C:1N, C:1N:1CA")
    lens = lengths_of(lengths_or_mask, L)
    if lens.shape != (B,):
        raise ValueError(f"{lens.shape[0]} lengths for a batch of {B}")
    sums, pairs = np.empty(B, np.float64), np.empty(B, np.int64)
    ca = np.empty((B, 2, L, 3), np.float64) if return_ca else None
    _binding.check(_binding.load().fd_pairwise_dist(int(device), _binding.ptr(a), _binding.ptr(c), _binding.ptr(p), _binding.ptr(k),
                                                    _binding.ptr(s), _binding.ptr(w), _binding.ptr(lens), B, L, F, _binding.ptr(idx),
                                                    _binding.ptr(sums), _binding.ptr(pairs), _binding.ptr(ca)))
    return (sums, pairs, ca) if return_ca else (sums, pairs)
