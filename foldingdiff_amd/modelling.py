"""
``BertForDiffusionBase`` -- drop-in for foldingdiff's noise-predictor object on
MI355X.  Same construction (``from_dir``), same attributes the callers touch
(``n_inputs``, ``parameters()``, ``.to()``, ``.eval()``, ``__call__``) and the
same ``forward(inputs, timestep, attention_mask)`` contract as
foldingdiff/modelling.py:211-484, but the arithmetic runs in libfdmi.so
(hand-written gfx950 kernels, include/fdmi.h).  There is no CPU path: calling
the model before ``.to("cuda")`` raises.

Differences from the reference, stated once:
* eval-mode only.  The reference samples with dropout active because
  ``bin/sample.py`` never calls ``.eval()``; parity here is defined against the
  deterministic eval-mode forward.
* prefix ``attention_mask``s (ones then zeros per row: what ``p_sample`` builds, sampling.py:56-58) run the tuned kernels;
  any other mask pattern and explicit ``position_ids`` are honoured too (``fd_forward_ex``, the general attention kernel).
* head size (hidden_size / num_attention_heads) 32 (every released configuration: the tuned kernels), 64, 96 or 128
  (a general kernel; the HuggingFace default BertConfig the reference's unit tests build has 64), default precision only;
  ``position_embedding_type`` one of ``absolute`` / ``relative_key`` / ``relative_key_query``.
"""
import ctypes as C
import glob
import json
import logging
import math
import os
import re
import shutil
from pathlib import Path
from typing import Dict, List, Literal, Optional, Sequence, Union

import numpy as np
import torch

from . import _binding, beta_schedules
from .datasets import FEATURE_SET_NAMES_TO_ANGULARITY, FEATURE_SET_NAMES_TO_FEATURE_NAMES

DEFAULT_PRECISION = "f16x3"  # fp16 hi/lo split on the fp16 matrix cores: fp32-class accuracy (measured <= the exact-fp32 kernels' error), > 2x faster
TIME_ENCODING = Literal["gaussian_fourier", "sinusoidal"]
DECODER_HEAD = Literal["mlp", "linear"]


class BertConfig:
    """The fields of HuggingFace ``BertConfig`` this path reads, loadable from the
    ``config.json`` that training writes (bin/train.py:463).  A real
    ``transformers.BertConfig`` is accepted wherever this class is."""

    def __init__(self, **kw):
        self.hidden_size = kw.pop("hidden_size", 768)
        self.num_attention_heads = kw.pop("num_attention_heads", 12)
        self.intermediate_size = kw.pop("intermediate_size", 3072)
        self.num_hidden_layers = kw.pop("num_hidden_layers", 12)
        self.max_position_embeddings = kw.pop("max_position_embeddings", 512)
        self.position_embedding_type = kw.pop("position_embedding_type", "absolute")
        self.layer_norm_eps = kw.pop("layer_norm_eps", 1e-12)
        self.hidden_act = kw.pop("hidden_act", "gelu")
        self.initializer_range = kw.pop("initializer_range", 0.02)
        self.hidden_dropout_prob = kw.pop("hidden_dropout_prob", 0.1)
        self.attention_probs_dropout_prob = kw.pop("attention_probs_dropout_prob", 0.1)
        self.is_decoder = kw.pop("is_decoder", False)
        self._extra = dict(kw)

    @classmethod
    def from_json_file(cls, path: str) -> "BertConfig":
        with open(path) as fh:
            return cls(**json.load(fh))

    def to_dict(self) -> dict:
        d = {k: v for k, v in self.__dict__.items() if not k.startswith("_")}
        d.update(self._extra)
        d.setdefault("model_type", "bert")
        return d

    def save_pretrained(self, dirname) -> None:
        os.makedirs(dirname, exist_ok=True)
        with open(os.path.join(dirname, "config.json"), "w") as fh:
            json.dump(self.to_dict(), fh, indent=2, sort_keys=True)


def gaussian_fourier_table(W: torch.Tensor, timesteps: int) -> torch.Tensor:
    """time_embed(t) for t = 0..T-1 exactly as GaussianFourierProjection.forward
    evaluates it (modelling.py:59-71): int64 t times the float32 buffer W, then *2,
    then *pi, all in float32 -- the sin/cos arguments reach ~1e5 rad, so the table is
    built on the host with the reference's op order instead of on the device."""
    t = torch.arange(timesteps, dtype=torch.long)
    proj = t[:, None] * W.detach().cpu().float()[None, :] * 2 * torch.pi
    return torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1).contiguous()


def sinusoidal_table(dim: int, timesteps: int) -> torch.Tensor:
    """SinusoidalPositionEmbeddings.forward (modelling.py:84-93) for t = 0..T-1."""
    half = dim // 2
    freq = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
    arg = torch.arange(timesteps, dtype=torch.long)[:, None] * freq[None, :]
    return torch.cat((arg.sin(), arg.cos()), dim=-1).contiguous()


def _param_names(cfg, n_inputs: int, decoder: str) -> Dict[str, tuple]:
    """state_dict names -> shapes, as BertForDiffusionBase.__init__ creates them
    (modelling.py:239-295 + HF BertEncoder)."""
    d, ff = cfg.hidden_size, cfg.intermediate_size
    names = {
        "inputs_to_hidden_dim.weight": (d, n_inputs),
        "inputs_to_hidden_dim.bias": (d,),
        "embeddings.LayerNorm.weight": (d,),
        "embeddings.LayerNorm.bias": (d,),
    }
    if cfg.position_embedding_type == "absolute":
        names["embeddings.position_embeddings.weight"] = (cfg.max_position_embeddings, d)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            names[p + f"attention.self.{n}.weight"] = (d, d)
            names[p + f"attention.self.{n}.bias"] = (d,)
        if cfg.position_embedding_type in ("relative_key", "relative_key_query"):
            names[p + "attention.self.distance_embedding.weight"] = (
                2 * cfg.max_position_embeddings - 1,
                d // cfg.num_attention_heads,
            )
        names[p + "attention.output.dense.weight"] = (d, d)
        names[p + "attention.output.dense.bias"] = (d,)
        names[p + "attention.output.LayerNorm.weight"] = (d,)
        names[p + "attention.output.LayerNorm.bias"] = (d,)
        names[p + "intermediate.dense.weight"] = (ff, d)
        names[p + "intermediate.dense.bias"] = (ff,)
        names[p + "output.dense.weight"] = (d, ff)
        names[p + "output.dense.bias"] = (d,)
        names[p + "output.LayerNorm.weight"] = (d,)
        names[p + "output.LayerNorm.bias"] = (d,)
    if decoder == "mlp":
        names["token_decoder.dense1.weight"] = (d, d)
        names["token_decoder.dense1.bias"] = (d,)
        names["token_decoder.layer_norm.weight"] = (d,)
        names["token_decoder.layer_norm.bias"] = (d,)
        names["token_decoder.dense2.weight"] = (n_inputs, d)
        names["token_decoder.dense2.bias"] = (n_inputs,)
    else:
        names["token_decoder.weight"] = (n_inputs, d)
        names["token_decoder.bias"] = (n_inputs,)
    return names


class BertForDiffusionBase:
    """BERT noise predictor for continuous angle inputs, executed by libfdmi.so."""

    def __init__(
        self,
        config,
        ft_is_angular: List[bool] = [False, True, True, True],
        ft_names: Optional[List[str]] = None,
        time_encoding: TIME_ENCODING = "gaussian_fourier",
        decoder: DECODER_HEAD = "mlp",
    ) -> None:
        self.config = config
        if getattr(config, "is_decoder", False):
            raise NotImplementedError
        self.ft_is_angular = list(ft_is_angular)
        self.n_inputs = len(self.ft_is_angular)
        self.ft_names = ft_names if ft_names is not None else [f"ft{i}" for i in range(self.n_inputs)]
        assert len(self.ft_names) == self.n_inputs
        if decoder not in ("mlp", "linear"):
            raise ValueError(f"Unrecognized decoder: {decoder}")
        if time_encoding not in ("gaussian_fourier", "sinusoidal"):
            raise ValueError(f"Unknown time encoding: {time_encoding}")
        if getattr(config, "hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"hidden_act={config.hidden_act!r}: only exact-erf 'gelu' is implemented")
        self.time_encoding = time_encoding
        self.decoder = decoder
        # what loss_terms reports (BertForDiffusion's loss / circle_reg / use_pairwise_dist_loss, modelling.py:492-543);
        # from_dir reads them from training_args.json, and all three may be set afterwards
        self.loss_key = "smooth_l1"
        self.circle_lambda = 0.0
        self.use_pairwise_dist_loss = 0.0
        # arithmetic of the GEMM kernels: "f32" (exact fp32 MFMA) or "f16x3" (fp16 hi/lo split
        # on the fp16 MFMA, fp32-class error); env FOLDINGDIFF_AMD_PRECISION overrides the default
        self.precision = os.environ.get("FOLDINGDIFF_AMD_PRECISION", DEFAULT_PRECISION)
        self.training = False
        self._device = torch.device("cpu")
        self._handle = None          # fd_model* on self._device
        self._tables_T = None        # T the device tables were finalised for
        self._betas_key = None
        self._param_cache = None
        # HF init_weights: N(0, initializer_range) matrices, zero bias, LayerNorm 1/0
        std = getattr(config, "initializer_range", 0.02)
        self._state: Dict[str, torch.Tensor] = {}
        for name, shape in _param_names(config, self.n_inputs, decoder).items():
            if name.endswith("LayerNorm.weight") or name.endswith("layer_norm.weight"):
                t = torch.ones(shape)
            elif name.endswith("bias"):
                t = torch.zeros(shape)
            else:
                t = torch.randn(shape) * std
            self._state[name] = t
        if time_encoding == "gaussian_fourier":
            self._state["time_embed.W"] = torch.randn(config.hidden_size // 2) * (2 * torch.pi)
        if config.position_embedding_type == "absolute":
            self._state["embeddings.position_ids"] = torch.arange(config.max_position_embeddings).expand((1, -1))

    # ------------------------------------------------------------------ loading
    @classmethod
    def from_dir(
        cls,
        dirname: str,
        ft_is_angular: Optional[Sequence[bool]] = None,
        load_weights: bool = True,
        idx: int = -1,
        best_by: Literal["train", "valid"] = "valid",
        copy_to: str = "",
        **kwargs,
    ):
        """Build the model from a training output directory: ``training_args.json``,
        ``config.json`` and ``models/best_by_{best_by}/*.ckpt`` (Lightning checkpoint
        with a ``state_dict`` key), same layout and arguments as modelling.py:297-382."""
        with open(os.path.join(dirname, "training_args.json")) as fh:
            train_args = json.load(fh)
        config = BertConfig.from_json_file(os.path.join(dirname, "config.json"))
        if ft_is_angular is None:
            ft_is_angular = FEATURE_SET_NAMES_TO_ANGULARITY[train_args["angles_definitions"]]
            logging.info(f"Auto constructed ft_is_angular: {ft_is_angular}")
        tkey = "time_encoding" if "time_encoding" in train_args else "seq_len_encoding"
        model = cls(config=config, ft_is_angular=ft_is_angular, time_encoding=train_args[tkey],
                    decoder=train_args["decoder"], **kwargs)
        # the loss the run was trained with (bin/train.py's loss, circle_reg, use_pdist_loss): what loss_terms reports
        model.set_loss(train_args.get("loss", "smooth_l1"), train_args.get("circle_reg", 0.0),
                       train_args.get("use_pdist_loss", 0.0))
        from . import losses
        if losses.pairwise_is_on(model.use_pairwise_dist_loss) and "ft_names" not in kwargs:
            # the pairwise term finds its six angles by name (bin/train.py hands the dataset's names to the model)
            model.ft_names = list(FEATURE_SET_NAMES_TO_FEATURE_NAMES[train_args["angles_definitions"]])
        ckpt_name = None
        subfolder = f"best_by_{best_by}"
        if load_weights:
            def epoch_of(p):
                return int(re.findall(r"epoch=[0-9]+", os.path.basename(p)).pop().split("=")[-1])

            ckpts = sorted(glob.glob(os.path.join(dirname, "models", subfolder, "*.ckpt")), key=epoch_of)
            logging.info(f"Found {len(ckpts)} checkpoints")
            ckpt_name = ckpts[idx]
            logging.info(f"Loading weights from {ckpt_name}")
            # Lightning checkpoints carry non-tensor metadata: trusted local file
            loaded = torch.load(ckpt_name, map_location=torch.device("cpu"), weights_only=False)
            model.load_state_dict(loaded["state_dict"])
        else:
            logging.info(f"Loaded unitialized model from {dirname}")
        if copy_to:
            dst = Path(copy_to)
            os.makedirs(dst, exist_ok=True)
            with open(dst / "training_args.json", "w") as fh:
                json.dump(train_args, fh)
            config.save_pretrained(dst)
            if load_weights:
                ckpt_dir = dst / "models" / subfolder
                os.makedirs(ckpt_dir, exist_ok=True)
                shutil.copyfile(ckpt_name, ckpt_dir / os.path.basename(ckpt_name))
        return model

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self._state)

    def load_state_dict(self, sd, strict: bool = True):
        want = set(self._state.keys())
        got = set(sd.keys())
        missing, unexpected = sorted(want - got), sorted(got - want)
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing}, unexpected {unexpected}")
        for k in want & got:
            v = sd[k].detach().cpu()
            if tuple(v.shape) != tuple(self._state[k].shape):
                raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)} vs {tuple(self._state[k].shape)}")
            self._state[k] = v.to(self._state[k].dtype).clone()
        self._invalidate()
        return self

    # --------------------------------------------------------- nn.Module surface
    def parameters(self):
        """Tensors on the model's device (callers do ``next(model.parameters()).device``)."""
        if self._device.type == "cpu":
            return iter(v for k, v in self._state.items() if v.is_floating_point() and k != "time_embed.W")
        if self._param_cache is None:
            self._param_cache = [v.to(self._device) for k, v in self._state.items()
                                 if v.is_floating_point() and k != "time_embed.W"]
        return iter(self._param_cache)

    @property
    def device(self) -> torch.device:
        return self._device

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            logging.warning("foldingdiff_amd runs the eval-mode forward only; train(True) is ignored")
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", 0)
        if device != self._device:
            self._invalidate()
            self._device = device
        return self

    def cuda(self, index: int = 0):
        return self.to(torch.device("cuda", index))

    def __del__(self):
        try:
            self._invalidate()
        except Exception:
            pass

    def _invalidate(self):
        if getattr(self, "_handle", None) is not None:
            _binding.load().fd_destroy(self._handle)
        self._handle = None
        self._tables_T = None
        self._betas_key = None
        self._param_cache = None

    # ----------------------------------------------------------- device model
    def _ensure_handle(self):
        if self._handle is not None:
            return self._handle
        if self._device.type != "cuda":
            raise RuntimeError(
                "foldingdiff_amd.BertForDiffusionBase computes only on an MI355X: call .to('cuda') first "
                "(there is no CPU fallback)."
            )
        lib = _binding.load()
        cfg = self.config
        if cfg.position_embedding_type not in _binding.FD_POS:
            raise NotImplementedError(f"position_embedding_type={cfg.position_embedding_type!r}")
        fc = _binding.FdConfig(
            n_features=self.n_inputs, d_model=cfg.hidden_size, n_heads=cfg.num_attention_heads,
            d_ff=cfg.intermediate_size, n_layers=cfg.num_hidden_layers, max_pos=cfg.max_position_embeddings,
            pos_type=_binding.FD_POS[cfg.position_embedding_type], decoder=_binding.FD_DEC[self.decoder],
            ln_eps=float(cfg.layer_norm_eps),
        )
        h = C.c_void_p()
        _binding.check(lib.fd_create(C.byref(fc), self._device.index or 0, C.byref(h)))
        try:
            for name, t in self._state.items():
                arr = np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32, copy=False))
                shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
                _binding.check(lib.fd_set_weight(h, name.encode(), _binding.ptr(arr), shape, arr.ndim))
        except Exception:
            lib.fd_destroy(h)
            raise
        self._handle = h
        return h

    def time_table(self, timesteps: int) -> torch.Tensor:
        if self.time_encoding == "gaussian_fourier":
            return gaussian_fourier_table(self._state["time_embed.W"], timesteps)
        return sinusoidal_table(self.config.hidden_size, timesteps)

    def prepare(self, betas: torch.Tensor, is_angle=None):
        """Upload the schedule / time tables for this beta schedule and the per-feature
        wrap flags (default: the model's ``ft_is_angular``).  No-op when unchanged."""
        h = self._ensure_handle()
        betas = betas.detach().to(device="cpu", dtype=torch.float32).contiguous()
        if is_angle is None:
            is_angle = self.ft_is_angular
        elif isinstance(is_angle, bool):
            is_angle = [is_angle] * self.n_inputs
        assert len(is_angle) == self.n_inputs
        if self.precision not in _binding.FD_PREC:
            raise ValueError(f"precision={self.precision!r}; expected one of {sorted(_binding.FD_PREC)}")
        key = (betas.numel(), betas.numpy().tobytes(), tuple(bool(a) for a in is_angle), self.precision)
        if self._betas_key == key:
            return h
        T = betas.numel()
        coef = np.ascontiguousarray(beta_schedules.step_coefficients(betas).numpy())
        table = np.ascontiguousarray(self.time_table(T).numpy().astype(np.float32))
        is_angle = np.ascontiguousarray(np.asarray(is_angle, dtype=np.uint8))
        _binding.check(_binding.load().fd_finalize(
            h, T, _binding.ptr(coef), _binding.ptr(table), _binding.ptr(is_angle), _binding.FD_PREC[self.precision]))
        self._betas_key = key
        self._tables_T = T
        return h

    def set_precision(self, precision: str):
        """Select the GEMM arithmetic ("f32" | "f16x3"); takes effect at the next prepare()."""
        if precision not in _binding.FD_PREC:
            raise ValueError(f"precision={precision!r}; expected one of {sorted(_binding.FD_PREC)}")
        if precision != self.precision:
            self.precision = precision
            self._betas_key = None
            self._tables_T = None
        return self

    def set_option(self, name: str, value: int):
        """fd_set_option; returns the value the option had before (0 if it was never set through this object)."""
        _binding.check(_binding.load().fd_set_option(self._ensure_handle(), name.encode(), int(value)))
        opts = self.__dict__.setdefault("_fd_options", {})
        prev = opts.get(name, 0)
        opts[name] = int(value)
        return prev

    def set_loss(self, loss: str = "smooth_l1", circle_reg: float = 0.0, use_pdist_loss=0.0):
        """The three loss settings of ``BertForDiffusion.__init__`` as ``loss_key``, ``circle_lambda`` and
        ``use_pairwise_dist_loss`` (a scalar, or ``(min_coef, max_coef, max_timesteps)``; a JSON list becomes the tuple),
        with the reference's autocorrection of the legacy key "radian_l1_smooth"."""
        from . import losses
        loss = losses.LOSS_AUTOCORRECT.get(loss, loss)
        if loss not in losses.LOSS_KINDS:
            raise ValueError(f"loss={loss!r}; expected one of {sorted(losses.LOSS_KINDS)}")
        self.loss_key = loss
        self.circle_lambda = float(circle_reg)
        self.use_pairwise_dist_loss = tuple(use_pdist_loss) if isinstance(use_pdist_loss, (list, tuple)) else float(use_pdist_loss)
        return self

    # ------------------------------------------------------------------ forward
    @staticmethod
    def lengths_from_mask(attention_mask: torch.Tensor) -> Optional[np.ndarray]:
        """Per-sequence lengths of a prefix mask (ones followed by zeros: what p_sample builds, sampling.py:56-58), or None when
        the mask has any other pattern (the forward then goes through fd_forward_ex and the general attention kernel)."""
        m = attention_mask.detach().cpu()
        assert m.dim() == 2, f"Attention mask expected in shape (batch_size, seq_length), got {m.shape}"
        lens = (m != 0).sum(dim=1)
        prefix = (torch.arange(m.shape[1])[None, :] < lens[:, None])
        if not torch.equal(prefix, m != 0) or int(lens.min()) < 1:
            return None
        return lens.numpy().astype(np.int32)

    def forward(self, inputs: torch.Tensor, timestep: torch.Tensor, attention_mask: torch.Tensor,
                position_ids: Optional[torch.Tensor] = None, **_unused) -> torch.Tensor:
        """eps = model(x, t, mask): [B, L, F] float32 -> [B, L, F] (modelling.py:384-484).
        Needs the time table: if ``prepare`` was never called, a table long enough for
        max(t)+1 steps is built with the default cosine schedule coefficients (the
        forward itself does not read them).

        Prefix masks with default position ids (everything the sampler produces) run the tuned kernels (``fd_forward``).  Any
        other ``attention_mask`` pattern and explicit ``position_ids`` (honoured with absolute position embeddings, as in the
        reference: modelling.py:434-442) go through ``fd_forward_ex``: same arithmetic, the general attention kernel."""
        assert attention_mask is not None
        assert inputs.dim() == 3
        B, L = int(inputs.shape[0]), int(inputs.shape[1])
        pids = None
        if position_ids is not None:
            want = torch.arange(L).expand(B, -1)
            try:  # (a broadcastable (1, L) / (L,) tensor is what callers usually pass)
                got = torch.broadcast_to(position_ids.detach().cpu().long(), want.shape)
            except RuntimeError:
                raise ValueError(f"position_ids of shape {tuple(position_ids.shape)} do not broadcast to ({B}, {L})")
            if not torch.equal(got, want) and self.config.position_embedding_type == "absolute":
                pids = np.ascontiguousarray(got.numpy().astype(np.int32))   # (relative types ignore them, as the reference does)
        lens = self.lengths_from_mask(attention_mask)
        t = timestep.detach().cpu().reshape(-1).long()
        assert t.numel() == B
        need_T = int(t.max()) + 1
        if self._tables_T is None or self._tables_T < need_T:
            self.prepare(beta_schedules.cosine_beta_schedule(max(need_T, 1000)))
        h = self._ensure_handle()
        lib = _binding.load()
        x = np.ascontiguousarray(inputs.detach().cpu().numpy().astype(np.float32))
        assert x.shape[2] == self.n_inputs
        kmask = None
        if lens is None or pids is not None:
            kmask = np.ascontiguousarray((attention_mask.detach().cpu() != 0).numpy().astype(np.uint8))
        out = np.empty_like(x)
        for tv in torch.unique(t).tolist():  # the device forward takes one t per launch
            rows = np.nonzero((t == tv).numpy())[0]
            xs = np.ascontiguousarray(x[rows])
            es = np.empty_like(xs)
            if kmask is None:
                ls = np.ascontiguousarray(lens[rows])
                _binding.check(lib.fd_forward(h, _binding.ptr(xs), int(tv), _binding.ptr(ls), len(rows), L, _binding.ptr(es)))
            else:
                ms = np.ascontiguousarray(kmask[rows])
                ps = np.ascontiguousarray(pids[rows]) if pids is not None else None
                _binding.check(lib.fd_forward_ex(h, _binding.ptr(xs), int(tv), _binding.ptr(ms), _binding.ptr(ps), len(rows), L,
                                                 _binding.ptr(es)))
            out[rows] = es
        return torch.from_numpy(out).to(inputs.device)

    __call__ = forward

    # ------------------------------------------------- one timestep per sequence, and the denoising loss
    def _batch_arrays(self, inputs: torch.Tensor, timestep: torch.Tensor, attention_mask: torch.Tensor):
        """(x float32 [B, L, F], t int32 [B], lens int32 [B]) of a batch with a prefix mask; the tables cover max(t)."""
        assert attention_mask is not None
        assert inputs.dim() == 3 and inputs.shape[2] == self.n_inputs
        B = int(inputs.shape[0])
        lens = self.lengths_from_mask(attention_mask)
        if lens is None:
            raise ValueError("one timestep per sequence is built for prefix masks (ones followed by zeros, at least one "
                             "position per sequence) only; forward() takes any mask, one launch per distinct timestep")
        t = timestep.detach().cpu().reshape(-1).long()
        if t.numel() != B:
            raise ValueError(f"{t.numel()} timesteps for a batch of {B}")
        need_T = int(t.max()) + 1
        if self._tables_T is None or self._tables_T < need_T:
            self.prepare(beta_schedules.cosine_beta_schedule(max(need_T, 1000)))
        x = np.ascontiguousarray(inputs.detach().cpu().numpy().astype(np.float32))
        return x, np.ascontiguousarray(t.numpy().astype(np.int32)), lens

    def forward_mixed_t(self, inputs: torch.Tensor, timestep: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """``forward`` for a batch whose sequences sit at different timesteps (a training / validation batch,
        modelling.py:553-566) as ONE device forward (``fd_forward_t``): sequence b adds ``time_embed(timestep[b])``.
        ``forward`` makes one launch sequence per distinct timestep instead.  With all timesteps equal the two return the
        same bits.  Prefix masks and default position ids only; anything else raises ``ValueError`` -- use ``forward``."""
        x, t, lens = self._batch_arrays(inputs, timestep, attention_mask)
        out = np.empty_like(x)
        _binding.check(_binding.load().fd_forward_t(self._ensure_handle(), _binding.ptr(x), _binding.ptr(t), _binding.ptr(lens),
                                                    x.shape[0], x.shape[1], _binding.ptr(out)))
        return torch.from_numpy(out).to(inputs.device)

    def denoise_loss_sums(self, x: torch.Tensor, noise: torch.Tensor, timestep: torch.Tensor, attention_mask: torch.Tensor,
                          keep: Optional[torch.Tensor] = None, spread: Optional[torch.Tensor] = None,
                          return_corrupted: bool = False, return_eps: bool = False):
        """``fd_denoise_loss``: float64 [B, F] sums over each sequence's unmasked positions of the smooth-L1 terms
        (``losses``: beta pi / 10 for angular features, 1 for the others) of the predicted noise against ``noise``.
        ``keep`` / ``spread`` ([B]: sqrt_alphas_cumprod_t, sqrt_one_minus_alphas_cumprod_t) given: ``x`` is the clean x_0
        and the device noises it (every position, angular features wrapped, the bits of ``NoisedAnglesDataset``); both
        None: ``x`` is the corrupted x_t already.  Returns ``sums``, or ``(sums, extras)`` with the requested
        ``"corrupted"`` / ``"eps"`` [B, L, F] arrays."""
        from . import losses
        if (keep is None) != (spread is None):
            raise ValueError("keep and spread go together")
        xa, t, lens = self._batch_arrays(x, timestep, attention_mask)
        B, L, F = xa.shape
        na = np.ascontiguousarray(noise.detach().cpu().numpy().astype(np.float32))
        if na.shape != xa.shape:
            raise ValueError(f"noise {na.shape} != x {xa.shape}")
        vec = lambda v: None if v is None else np.ascontiguousarray(torch.as_tensor(v).detach().cpu().reshape(-1).numpy().astype(np.float32))  # noqa: E731
        ka, sa = vec(keep), vec(spread)
        if ka is not None and (ka.shape != (B,) or sa.shape != (B,)):
            raise ValueError(f"keep / spread must hold one value per sequence ({B})")
        sums = np.empty((B, F), np.float64)
        corrupted = np.empty_like(xa) if return_corrupted else None
        eps = np.empty_like(xa) if return_eps else None
        _binding.check(_binding.load().fd_denoise_loss(
            self._ensure_handle(), _binding.ptr(xa), _binding.ptr(na), _binding.ptr(t), _binding.ptr(ka), _binding.ptr(sa),
            _binding.ptr(lens), B, L, float(losses.ANGULAR_BETA), float(losses.NONANGULAR_BETA), _binding.ptr(sums),
            _binding.ptr(corrupted), _binding.ptr(eps)))
        if return_corrupted or return_eps:
            return sums, {k: v for k, v in (("corrupted", corrupted), ("eps", eps)) if v is not None}
        return sums

    def denoise_loss_ex(self, x0: torch.Tensor, noise: torch.Tensor, timestep: torch.Tensor, attention_mask: torch.Tensor,
                        corrupted: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                        spread: Optional[torch.Tensor] = None, kind: Union[int, str] = 0, return_turns: bool = False,
                        pairwise: bool = False, coef=None, return_corrupted: bool = False, return_eps: bool = False) -> Dict[str, np.ndarray]:
        """``fd_denoise_loss_ex``: ``denoise_loss_sums`` with the loss kind (0 / "smooth_l1", 1 / "l1"), the turn counts
        of the circle penalty and the pairwise-distance sums of the forward's own prediction -- one upload, one small
        download, the prediction never leaves the device.  ``x0`` is the clean batch; ``corrupted`` None: the device
        noises it with ``keep`` / ``spread``.  ``pairwise=True`` needs ``keep`` / ``spread`` and a feature set with the
        six angles; ``coef``: None, a scalar, or one weight per sequence.  Returns a dict: ``"sums"`` float64 [B, F],
        and where asked for ``"turns"`` int64 [B, F], ``"pair_sums"`` float64 [B] with ``"pairs"`` int64 [B],
        ``"corrupted"`` / ``"eps"`` float32 [B, L, F]."""
        from . import losses
        kind = losses.LOSS_KINDS[kind] if isinstance(kind, str) else int(kind)
        if (keep is None) != (spread is None):
            raise ValueError("keep and spread go together")
        if corrupted is None and keep is None:
            raise ValueError("without corrupted the device noises x0 and needs keep and spread")
        if pairwise and keep is None:
            raise ValueError("the pairwise-distance term needs keep and spread (sqrt_alphas_cumprod_t, sqrt_one_minus_alphas_cumprod_t)")
        idx = losses.pairwise_columns(self.ft_names) if pairwise else None
        xa, t, lens = self._batch_arrays(x0, timestep, attention_mask)
        B, L, F = xa.shape
        f32 = lambda v: np.ascontiguousarray(torch.as_tensor(v).detach().cpu().numpy().astype(np.float32))  # noqa: E731
        na = f32(noise)
        ca = None if corrupted is None else f32(corrupted)
        if na.shape != xa.shape or (ca is not None and ca.shape != xa.shape):
            raise ValueError(f"noise {na.shape} / corrupted {None if ca is None else ca.shape} != x0 {xa.shape}")
        vec = lambda v: None if v is None else np.ascontiguousarray(f32(v).reshape(-1))  # noqa: E731
        ka, sa, wa = vec(keep), vec(spread), vec(coef)
        if ka is not None and (ka.shape != (B,) or sa.shape != (B,)):
            raise ValueError(f"keep / spread must hold one value per sequence ({B})")
        if wa is not None:
            wa = np.ascontiguousarray(np.broadcast_to(wa, (B,))) if wa.size == 1 else wa
            if wa.shape != (B,):
                raise ValueError(f"coef must be a scalar or hold one value per sequence ({B})")
        out = {"sums": np.empty((B, F), np.float64)}
        if return_turns:
            out["turns"] = np.empty((B, F), np.int64)
        if pairwise:
            out["pair_sums"], out["pairs"] = np.empty(B, np.float64), np.empty(B, np.int64)
        if return_corrupted:
            out["corrupted"] = np.empty_like(xa)
        if return_eps:
            out["eps"] = np.empty_like(xa)
        P = _binding.ptr
        _binding.check(_binding.load().fd_denoise_loss_ex(
            self._ensure_handle(), P(xa), P(ca), P(na), P(t), P(ka), P(sa), P(lens), B, L, kind, float(losses.ANGULAR_BETA),
            float(losses.NONANGULAR_BETA), P(wa if pairwise else None), P(idx), P(out["sums"]), P(out.get("turns")),
            P(out.get("pair_sums")), P(out.get("pairs")), P(out.get("corrupted")), P(out.get("eps"))))
        return out

    def loss_terms(self, batch) -> torch.Tensor:
        """``BertForDiffusion._get_loss_terms(batch)`` (modelling.py:553-679) under the model's ``loss_key``,
        ``circle_lambda`` and ``use_pairwise_dist_loss``: a float64 [F] tensor, per feature the mean over all unmasked
        positions of the batch of the term of the predicted against the known noise (smooth L1 or l1; angular features
        wrapped), plus ``circle_lambda`` times the mean turn count of the predicted noise for angular features under
        "smooth_l1"; with the pairwise-distance term on, [F + 1]: the last entry is the mean over all CA pairs of the
        batch of the weighted squared distance difference between the chains of the clean and of the denoised angles
        (NaN when no sequence has two residues).  ``batch`` has the reference's keys ``corrupted``, ``t``,
        ``known_noise`` and ``attn_mask`` (a prefix mask), and with the pairwise term also ``angles``, ``lengths``,
        ``sqrt_alphas_cumprod_t`` and ``sqrt_one_minus_alphas_cumprod_t``.  One device call: forward with one timestep
        per sequence, terms and per-sequence fp64 sums; the means are taken here in float64 (the reference's are float32
        ``torch.mean``s)."""
        from . import losses
        pairwise = losses.pairwise_is_on(self.use_pairwise_dist_loss)
        circle = self.loss_key == "smooth_l1" and self.circle_lambda > 0
        need = ["corrupted", "t", "known_noise", "attn_mask"]
        if pairwise:
            need += ["angles", "lengths", "sqrt_alphas_cumprod_t", "sqrt_one_minus_alphas_cumprod_t"]
        missing = [k for k in need if k not in batch]
        if missing:
            raise KeyError(f"loss_terms: the batch lacks {missing}" + (" (needed by the pairwise-distance loss)" if pairwise else ""))
        count = int((batch["attn_mask"].detach().cpu() != 0).sum())
        if self.loss_key == "smooth_l1" and not circle and not pairwise:
            sums = self.denoise_loss_sums(batch["corrupted"], batch["known_noise"], batch["t"], batch["attn_mask"])
            return torch.from_numpy(sums.sum(axis=0) / count)
        if pairwise:
            lens = self.lengths_from_mask(batch["attn_mask"])
            given = torch.as_tensor(batch["lengths"]).detach().cpu().reshape(-1).numpy()
            if lens is None or not np.array_equal(lens, given):
                raise ValueError("batch['lengths'] and the prefix mask batch['attn_mask'] disagree")
            coef = losses.pairwise_coef(self.use_pairwise_dist_loss, batch["t"].detach().cpu())
            out = self.denoise_loss_ex(batch["angles"], batch["known_noise"], batch["t"], batch["attn_mask"],
                                       corrupted=batch["corrupted"], keep=batch["sqrt_alphas_cumprod_t"],
                                       spread=batch["sqrt_one_minus_alphas_cumprod_t"], kind=self.loss_key, return_turns=circle,
                                       pairwise=True, coef=coef)
        else:
            out = self.denoise_loss_ex(batch["corrupted"], batch["known_noise"], batch["t"], batch["attn_mask"],
                                       corrupted=batch["corrupted"], kind=self.loss_key, return_turns=circle)
        terms = out["sums"].sum(axis=0) / count
        if circle:
            terms = terms + self.circle_lambda * (out["turns"].sum(axis=0).astype(np.float64) / count)
        if pairwise:
            n_pairs = int(out["pairs"].sum())
            terms = np.append(terms, out["pair_sums"].sum() / n_pairs if n_pairs else np.nan)
        return torch.from_numpy(terms)


class BertForAutoregressiveBase(BertForDiffusionBase):
    """The autoregressive baseline (foldingdiff/modelling.py:807-893): the same network, checkpoint layout and ``from_dir``,
    with the time embedding reused as an embedding of each sequence's target length -- added to the input projection
    *before* the position embedding and the embeddings LayerNorm -- and a sampler that predicts one residue per step from
    the residues before it.  Runs on the row-image kernels (precision "f16x3") only."""

    def prepare(self, is_angle=None):
        """Upload the length table: ``time_embed(n)`` for n = 0 .. max_position_embeddings, built like the diffusion
        model's time table.  There is no schedule; the coefficient rows ``fd_finalize`` wants are those of a cosine
        schedule of the same size, and nothing on this path reads them."""
        T = int(self.config.max_position_embeddings) + 1
        return super().prepare(beta_schedules.cosine_beta_schedule(T), is_angle=is_angle)

    def _lengths(self, seq_lengths, B: int) -> np.ndarray:
        n = torch.as_tensor(seq_lengths).detach().cpu().reshape(-1).long()
        if n.numel() != B:
            raise ValueError(f"{n.numel()} sequence lengths for a batch of {B}")
        T = int(self.config.max_position_embeddings) + 1
        if int(n.min()) < 0 or int(n.max()) >= T:
            raise ValueError(f"seq_lengths must lie in [0, {T}): the length table has max_position_embeddings + 1 rows")
        return np.ascontiguousarray(n.numpy().astype(np.int32))

    def forward(self, inputs: torch.Tensor, attention_mask: torch.Tensor, seq_lengths: torch.Tensor,
                position_ids: Optional[torch.Tensor] = None, **_unused) -> torch.Tensor:
        """``forward(inputs, attention_mask, seq_lengths)`` of the reference (modelling.py:812-862): [B, L, F] -> [B, L, F],
        every position computed.  Prefix masks (ones followed by zeros, at least one position per sequence) only."""
        assert attention_mask is not None
        assert inputs.dim() == 3 and inputs.shape[2] == self.n_inputs
        if position_ids is not None:
            raise NotImplementedError("explicit position_ids are not implemented for the autoregressive forward")
        B, L = int(inputs.shape[0]), int(inputs.shape[1])
        key_lens = self.lengths_from_mask(attention_mask)
        if key_lens is None:
            raise NotImplementedError("the autoregressive forward takes prefix masks only (ones followed by zeros, at least "
                                      "one position per sequence): what sample() builds")
        lens = self._lengths(seq_lengths, B)
        h = self.prepare()
        x = np.ascontiguousarray(inputs.detach().cpu().numpy().astype(np.float32))
        out = np.empty_like(x)
        _binding.check(_binding.load().fd_ar_forward(h, _binding.ptr(x), _binding.ptr(lens), _binding.ptr(key_lens), B, L,
                                                     _binding.ptr(out)))
        return torch.from_numpy(out).to(inputs.device)

    __call__ = forward

    def sample(self, seed_angles: torch.Tensor, seq_lengths: torch.Tensor, num_seed: int = 2,
               pbar: bool = True) -> List[torch.Tensor]:
        """``sample`` of the reference (modelling.py:864-893): the first ``num_seed`` positions of ``seed_angles``
        [B, L, F] are kept, position i = num_seed .. max(seq_lengths) - 1 becomes row i of the forward over the positions
        before it (row i itself enters with what ``seed_angles`` holds there), and sequence b is returned trimmed to
        ``seq_lengths[b]``.  The whole loop is one device call (``fd_ar_sample``), so there is nothing for ``pbar`` to show;
        it is accepted for the signature."""
        assert torch.all(seed_angles[:, :num_seed, :] <= torch.pi)
        assert torch.all(seed_angles[:, :num_seed, :] >= -torch.pi)
        assert seed_angles.ndim == 3 and seed_angles.shape[2] == self.n_inputs
        B, L = int(seed_angles.shape[0]), int(seed_angles.shape[1])
        if num_seed < 1:
            raise ValueError("num_seed must be at least 1: without a seed the first position would see masked keys only")
        lens = self._lengths(seq_lengths, B)
        if int(lens.max()) > L:
            raise ValueError(f"max(seq_lengths)={int(lens.max())} exceeds the {L} positions of seed_angles")
        h = self.prepare()
        x = np.ascontiguousarray(seed_angles.detach().cpu().numpy().astype(np.float32))
        out = np.empty_like(x)
        _binding.check(_binding.load().fd_ar_sample(h, _binding.ptr(x), _binding.ptr(lens), B, L, int(num_seed), _binding.ptr(out)))
        ret = torch.from_numpy(out).to(seed_angles.device)
        return [ret[i, :n, :] for i, n in enumerate(lens.tolist())]


# The reference's sampling entry points take the Lightning subclass or the base
# class interchangeably; only the base (inference) surface exists here.
BertForDiffusion = BertForDiffusionBase
BertForAutoregressive = BertForAutoregressiveBase
