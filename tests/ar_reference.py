"""
CPU restatement of the autoregressive baseline (TEST INFRASTRUCTURE ONLY): ``BertForAutoregressiveBase.forward`` and
``.sample`` (foldingdiff/modelling.py:807-893) composed from the oracle's own modules (``oracle.ref_model``), which stay
as they are.  The network is the diffusion model's; what differs is where the time embedding -- here the embedding of
each sequence's target length -- enters: before the position embedding and the embeddings LayerNorm, and nothing after.
"""
import copy

import torch


@torch.no_grad()
def ar_forward(om, inputs, attention_mask, seq_lengths):
    """modelling.py:812-862 on an ``OracleBertForDiffusion``; float32 or float64 by the model's and the inputs' dtype."""
    assert inputs.dim() == 3 and attention_mask.dim() == 2
    b, l = inputs.shape[:2]
    h = om.inputs_to_hidden_dim(inputs)                                       # :823
    h = h + om.time_encode(torch.as_tensor(seq_lengths), h.dtype).unsqueeze(1)  # :827-828
    position_ids = torch.arange(l).expand(b, -1)                              # :830-839
    ext = (1.0 - attention_mask[:, None, None, :].to(inputs.dtype)) * -10000.0  # :847-849
    h = om.embeddings(h, position_ids=position_ids)                           # :851
    return om.token_decoder(om.encoder(h, ext))                               # :852-862


@torch.no_grad()
def ar_sample(om, seed_angles, seq_lengths, num_seed=2, return_full=False):
    """modelling.py:864-893: the square loop, every step a forward over all L positions.  ``return_full``: the final
    [B, L, F] state instead of the trimmed list."""
    seq_lengths = torch.as_tensor(seq_lengths)
    assert torch.all(seed_angles[:, :num_seed, :] <= torch.pi)
    assert torch.all(seed_angles[:, :num_seed, :] >= -torch.pi)
    assert seed_angles.ndim == 3
    retval = seed_angles.clone()
    mask = torch.zeros(seed_angles.shape[:2], dtype=seed_angles.dtype)
    for i in range(num_seed, int(seq_lengths.max())):
        mask[:, :i] = 1.0
        retval[:, i, :] = ar_forward(om, retval, mask, seq_lengths)[:, i, :]
    if return_full:
        return retval
    return [retval[i, :n, :] for i, n in enumerate(seq_lengths.tolist())]


def as_double(om32, n_table):
    """A float64 copy of a float32 oracle whose time table holds the float32 values of rows 0 .. n_table-1: the sin / cos
    arguments are large, and the table is an input of the device path, not something it computes."""
    om64 = copy.deepcopy(om32).double()
    om64.time_table = om32.time_embed(torch.arange(n_table)).double()
    return om64


def prefix_mask(key_lens, L, dtype=torch.float32):
    m = torch.zeros(len(key_lens), L, dtype=dtype)
    for i, n in enumerate(key_lens):
        m[i, :n] = 1.0
    return m
