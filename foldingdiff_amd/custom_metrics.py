"""
The reference's ``custom_metrics`` (foldingdiff/custom_metrics.py): histogram KL divergences of angle distributions and
the wrapped mean, with the counting on the device where there is a lot of it.

* ``kl_from_empirical(u, v)``: KL(u || v) of two samples over ``nbins`` equal bins between their joint min and max -- the
  number ``bin/sample_plotting_only.py`` logs per angle as ``KL(generated || test)``.
* ``kl_from_dset(dset)``: for every timestep, every residue of the dataset noised to that timestep against a draw of the
  prior of the same size, per feature -- ``bin/train.py``'s ``kl_divergence_timesteps.pdf``, the check that T steps of a
  schedule reach the prior.  Two device passes over all timesteps at once (``fd_noise_minmax``, ``fd_noise_hist``); only
  min / max and integer counts leave the device.
* ``wrapped_mean``, ``angle_kl_report``.

What is restated and what is not: the bin edges are ALWAYS numpy's own ``np.linspace`` of the inputs' min and max, in the
dtype numpy gives them, computed on the host; the device only counts against them (widened to float64, which changes no
comparison).  ``np.histogram``'s bin rule and its ``density=True`` normalisation are restated (``hist_columns``,
``_density``), and so is ``scipy.stats.entropy(pk, qk)`` (``relative_entropy``): scipy is not a dependency.
"""
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _binding
from ._binding import ptr

HIST_MAX_BINS = 4096   # FDMI_HIST_MAX_BINS


def relative_entropy(pk: np.ndarray, qk: np.ndarray) -> float:
    """``scipy.stats.entropy(pk, qk)``: both normalised to sum 1, then the sum of p log(p / q) where p > 0 and q > 0, 0
    where p == 0, inf where p > 0 and q == 0 (NaN stays NaN)."""
    pk, qk = np.asarray(pk, dtype=np.float64), np.asarray(qk, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pk = 1.0 * pk / np.sum(pk)
        qk = 1.0 * qk / np.sum(qk)
        both = (pk > 0) & (qk > 0)
        vec = np.where(both, pk * np.log(np.where(both, pk / qk, 1.0)), np.where((pk == 0) & (qk >= 0), 0.0, np.inf))
        vec = np.where(np.isnan(pk) | np.isnan(qk), np.nan, vec)
    return np.sum(vec)


def _density(counts: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """What ``np.histogram(..., density=True)`` makes of its integer counts: n / diff(edges) / n.sum(), the widths taken in
    the edges' own dtype and then widened."""
    n = np.asarray(counts, dtype=np.intp)
    with np.errstate(divide="ignore", invalid="ignore"):
        return n / np.array(np.diff(edges), float) / n.sum()


def hist_columns(values: np.ndarray, edges: np.ndarray, device: int = 0,
                 rows_valid: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``np.histogram(values[:, f], bins=edges[f])[0]`` for every column f of a float32 [N, F] table, on the device
    (``fd_hist_columns``): int64 ``counts`` [F, nbins] and ``outside`` [F], the values of a column that are in none of
    its bins.  ``edges``: [F, nbins + 1], non-decreasing rows of any float dtype (widened to float64, which is exact).
    ``rows_valid``: optional boolean [N], rows to count."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    if values.ndim != 2 or edges.ndim != 2 or edges.shape[0] != values.shape[1]:
        raise ValueError(f"values {values.shape} and edges {edges.shape}: want [N, F] and [F, nbins + 1]")
    N, F = values.shape
    nbins = edges.shape[1] - 1
    valid = None
    if rows_valid is not None:
        valid = np.ascontiguousarray(rows_valid, dtype=np.uint8)
        if valid.shape != (N,):
            raise ValueError(f"rows_valid {valid.shape}: want [{N}]")
    counts, outside = np.empty((F, max(nbins, 0)), np.int64), np.empty((F,), np.int64)
    _binding.check(_binding.load().fd_hist_columns(device, ptr(values), N, F, ptr(edges), nbins, ptr(valid), ptr(counts),
                                                   ptr(outside)))
    return counts, outside


def kl_from_empirical(u: np.ndarray, v: np.ndarray, nbins: int = 100, pseudocount: bool = False,
                      device: Optional[int] = None) -> float:
    """KL(u || v) of two 1-D samples discretised into ``nbins`` equal bins between their joint min and max
    (foldingdiff/custom_metrics.py:15-37).  ``pseudocount`` appends every bin edge to both samples, so every bin gets one
    more count and the last one two.

    ``device=None`` counts with ``np.histogram``.  With a device, float32 samples are counted by ``fd_hist_columns``
    against the same edges (the pseudocounts added on the host); a degenerate range (min == max), samples of another
    dtype and more than 4096 bins take the host path.  Both paths give the same counts, so the same value."""
    u, v = np.asarray(u), np.asarray(v)
    min_val = min(np.min(u), np.min(v))
    max_val = max(np.max(u), np.max(v))
    bins = np.linspace(min_val, max_val, nbins + 1)
    on_device = (device is not None and u.dtype == np.float32 and v.dtype == np.float32 and u.ndim == 1 and v.ndim == 1
                 and min_val < max_val and 1 <= nbins <= HIST_MAX_BINS)
    if not on_device:
        if pseudocount:
            u = np.concatenate((u, bins))
            v = np.concatenate((v, bins))
        with np.errstate(divide="ignore", invalid="ignore"):
            u_hist, _ = np.histogram(u, bins=bins, density=True)
            v_hist, _ = np.histogram(v, bins=bins, density=True)
        return relative_entropy(u_hist, v_hist)
    counts = []
    for sample in (u, v):
        n, outside = hist_columns(sample[:, None], bins[None, :], device=device)
        assert outside[0] == 0 and n.sum() == sample.size, "a value outside its own min .. max"
        counts.append(n[0])
    if pseudocount:
        extra = np.histogram(bins, bins=bins)[0]   # the appended edges: one per bin, two in the last
        counts = [n + extra for n in counts]
    return relative_entropy(_density(counts[0], bins), _density(counts[1], bins))


def wrapped_mean(x: np.ndarray, axis=None) -> float:
    """The mean of angles on the circle, in [-pi, pi], ignoring NaN (foldingdiff/custom_metrics.py:82-94)."""
    return np.arctan2(np.nanmean(np.sin(x), axis=axis), np.nanmean(np.cos(x), axis=axis))


def angle_kl_report(sampled: np.ndarray, test: np.ndarray, feature_names: Sequence[str], nbins: int = 200,
                    pseudocount: bool = True, device: Optional[int] = None) -> Dict[str, float]:
    """{feature: KL(generated || test)} for the columns of ``sampled`` [N, F] and ``test`` [M, F], with the bins and the
    pseudocount of the reference's report (bin/sample_plotting_only.py:105-110)."""
    sampled, test = np.asarray(sampled), np.asarray(test)
    if sampled.ndim != 2 or test.ndim != 2 or sampled.shape[1] != len(feature_names) or test.shape[1] != len(feature_names):
        raise ValueError(f"sampled {sampled.shape}, test {test.shape}: want [N, {len(feature_names)}] and [M, {len(feature_names)}]")
    return {name: float(kl_from_empirical(np.ascontiguousarray(sampled[:, i]), np.ascontiguousarray(test[:, i]), nbins=nbins,
                                          pseudocount=pseudocount, device=device))
            for i, name in enumerate(feature_names)}


def stack_unmasked(dset) -> np.ndarray:
    """The unmasked rows of every item of the dataset ``dset`` wraps, as the dataset returns them (zero-centred when it
    centres), stacked into one float32 [N, F] table."""
    rows = []
    for i in range(len(dset.dset)):
        item = dset.dset.__getitem__(i)
        vals = item[dset.dset_key] if dset.dset_key is not None else item
        rows.append(np.asarray(vals, dtype=np.float32)[np.asarray(item["attn_mask"]) != 0])
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def _noise_tables(dset):
    """is_angle (uint8 [F]), scale (float32 [F]), keep and spread (float32 [T]) of a ``NoisedAnglesDataset``."""
    angular = np.array(dset.feature_is_angular[dset.dset_key], dtype=np.uint8)
    scale = np.where(angular != 0, np.float32(dset.angular_var_scale), np.float32(dset.nonangular_var_scale)).astype(np.float32)
    terms = dset.alpha_beta_terms
    keep = np.ascontiguousarray(terms["sqrt_alphas_cumprod"].float().numpy())
    spread = np.ascontiguousarray(terms["sqrt_one_minus_alphas_cumprod"].float().numpy())
    return angular, scale, keep, spread


def kl_from_dset(dset, timesteps: Optional[Sequence[int]] = None, nbins: int = 100, seed: int = 6489,
                 batch_rows: Optional[int] = None, device: int = 0, noise: Optional[Tuple[np.ndarray, np.ndarray]] = None,
                 return_draws: bool = False):
    """float64 [len(timesteps), F]: per timestep and feature, KL(noised data || prior draw) of ``kl_from_empirical`` with
    its defaults' bin rule -- ``custom_metrics.kl_from_dset`` (foldingdiff/custom_metrics.py:40-78).  ``dset`` is a
    ``NoisedAnglesDataset`` over a dataset with items (``structures.PdbAnglesDataset``); its schedule,
    ``angular_var_scale`` and ``nonangular_var_scale`` are honoured.  ``timesteps``: default all of them.

    The unmasked rows of every item are stacked once.  Pass 1 (``fd_noise_minmax``) noises every row to every timestep
    (``x_t``), draws the comparison sample (``cmp``) and returns their min and max; the host makes ``np.linspace`` edges
    per (timestep, feature) over min(x_t, cmp) .. max(x_t, cmp); pass 2 (``fd_noise_hist``) regenerates both streams and
    counts them; the KL is taken on the host.  That nothing fell outside the edges and every histogram sums to N is
    asserted: it shows the passes saw the same streams.  ``batch_rows`` bounds the rows of one device call.

    The draws are Philox streams under two seeds derived from ``seed``, not the reference's ``torch.randn`` stream: the
    result is the same statistic as the reference's on different draws, not the same digits.  ``noise=(eps, cmp)``,
    float32 [len(timesteps), N, F] each as ``sample_noise`` returns them (scaled and wrapped), reproduces given draws.
    ``return_draws``: also return ``x_t`` and ``cmp`` ([len(timesteps), N, F]; small N only)."""
    values = stack_unmasked(dset)
    if not np.isfinite(values).all():
        raise ValueError("the dataset holds non-finite features")
    N, F = values.shape
    ts = np.arange(dset.timesteps, dtype=np.int32) if timesteps is None else np.asarray(list(timesteps), dtype=np.int32)
    if ts.ndim != 1 or ts.size < 1 or ts.min() < 0 or ts.max() >= dset.timesteps:
        raise ValueError(f"timesteps outside [0, {dset.timesteps})")
    if not 1 <= nbins <= HIST_MAX_BINS:
        raise ValueError(f"nbins={nbins} outside [1, {HIST_MAX_BINS}]")
    nT = int(ts.size)
    angular, scale, keep, spread = _noise_tables(dset)
    assert angular.size == F
    eps_all = cmp_all = None
    if noise is not None:
        eps_all, cmp_all = (np.asarray(a, dtype=np.float32) for a in noise)
        if eps_all.shape != (nT, N, F) or cmp_all.shape != (nT, N, F):
            raise ValueError(f"noise {eps_all.shape}, {cmp_all.shape}: want two [{nT}, {N}, {F}]")
    seed_eps, seed_cmp = (int(s) for s in np.random.SeedSequence(seed).generate_state(2, np.uint64))
    step = N if batch_rows is None else int(batch_rows)
    if step < 1:
        raise ValueError(f"batch_rows={batch_rows}")
    lib = _binding.load()

    def batches():
        for r0 in range(0, N, step):
            r1 = min(N, r0 + step)
            given = [None if a is None else np.ascontiguousarray(a[:, r0:r1]) for a in (eps_all, cmp_all)]
            yield r0, np.ascontiguousarray(values[r0:r1]), given

    def common(r0, x0, given):
        return (device, ptr(x0), x0.shape[0], F, ptr(angular), ptr(scale), ptr(keep), ptr(spread), keep.size, ptr(ts), nT,
                seed_eps, seed_cmp, r0, ptr(given[0]), ptr(given[1]))

    lo = np.full((nT, F), np.inf, np.float32)
    hi = np.full((nT, F), -np.inf, np.float32)
    for r0, x0, given in batches():
        mm = np.empty((nT, 2, F, 2), np.float32)
        _binding.check(lib.fd_noise_minmax(*common(r0, x0, given), ptr(mm)))
        lo = np.minimum(lo, mm[..., 0].min(axis=1))
        hi = np.maximum(hi, mm[..., 1].max(axis=1))
    # numpy's own edges for these float32 bounds, in the dtype numpy gives them
    native = [[np.linspace(lo[i, f], hi[i, f], nbins + 1) for f in range(F)] for i in range(nT)]
    edges = np.ascontiguousarray(np.array(native, dtype=np.float64))
    counts = np.zeros((nT, 2, F, nbins), np.int64)
    draws = ([], [])
    for r0, x0, given in batches():
        part, outside = np.empty_like(counts), np.empty((nT, 2, F), np.int64)
        outs = [np.empty((nT, x0.shape[0], F), np.float32) if return_draws else None for _ in range(2)]
        _binding.check(lib.fd_noise_hist(*common(r0, x0, given), ptr(edges), nbins, ptr(part), ptr(outside), ptr(outs[0]),
                                         ptr(outs[1]), None))
        assert not outside.any(), "pass 2 drew a value outside pass 1's min .. max"
        counts += part
        if return_draws:
            draws[0].append(outs[0])
            draws[1].append(outs[1])
    assert (counts.sum(axis=3) == N).all(), "a histogram does not sum to the number of rows"
    kl = np.array([[relative_entropy(_density(counts[i, 0, f], native[i][f]), _density(counts[i, 1, f], native[i][f]))
                    for f in range(F)] for i in range(nT)], dtype=np.float64)
    if return_draws:
        return kl, np.concatenate(draws[0], axis=1), np.concatenate(draws[1], axis=1)
    return kl
