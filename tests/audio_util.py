"""Shared by the audio tests and tests/golden/make_golden_audio.py: the deterministic parameters and inputs of the audio goldens.

The oracle does not know audio (oracle/bist_oracle.py asserts nb_aenc_blocks == 0), so parameters are regenerated from the REFERENCE
model's own state_dict names and shapes, which the golden file stores as a list: ``O.det_param(name, shape)`` per name, the shared
embedding under its canonical name.  The audio input comes from a seed stored in the file.
"""
import argparse
import json

import numpy as np
import torch

from oracle import bist_oracle as O

LUT = "query_embed.0.lut.weight"
LUT_ALIASES = ("tgt_embed.0.lut.weight", "generator.vocab_gen", "ae_generator.proj")       # one tensor in the model (mtn.py:82,90,101)


def audio_state(names_shapes):
    """name -> deterministic tensor for a list of (name, shape); the positional-encoding buffers are left out."""
    sd = {}
    for name, shape in names_shapes:
        if name.endswith(".pe"):
            continue
        sd[name] = O.det_param(LUT if name in LUT_ALIASES else name, tuple(shape))
    return sd


def audio_input(B, Ta, Da, seed, zero_tail=((1, 3),), zero_sum_row=None):
    """N(0,1) audio features [B, Ta, Da]; zero_tail: (clip, n) pairs -- the clip's last n rows are all zero; zero_sum_row: (clip, row)
    whose entries are +1, -1, 0, ...: non-zero, yet summing to exactly 0.0 (the reference masks it: dataset.py:87)."""
    au = np.random.RandomState(seed).standard_normal((B, Ta, Da)).astype(np.float32)
    for clip, n in zero_tail:
        if clip < B and n < Ta:
            au[clip, Ta - n:] = 0.0
    if zero_sum_row is not None:
        clip, row = zero_sum_row
        au[clip, row] = 0.0
        au[clip, row, 0], au[clip, row, 1] = 1.0, -1.0
    return au


def cfg_args(cfg_dict):
    """The argparse.Namespace make_model reads, from a stored cfg dict (no noW_venc: absent counts as false)."""
    return argparse.Namespace(**{**cfg_dict, "d_ff": 4 * cfg_dict["d_model"]})


def case_meta(g, tag):
    return json.loads(str(g[f"{tag}_cfg"]))


def case_batch(meta):
    """(OBatch, audio numpy) of a stored case."""
    dm = meta["dims"]
    ob = O.det_batch(dm["B"], dm["T"], dm["S"], dm["C"], dm["Lq"], dm["Lh"], dm["Lc"], dm["Lt"], dm["V"], seed=dm.get("seed", 1234))
    au = audio_input(dm["B"], dm["Ta"], dm["Da"], dm["audio_seed"], zero_tail=[tuple(z) for z in dm.get("zero_tail", [[1, 3]])],
                     zero_sum_row=tuple(dm["zero_sum_row"]) if dm.get("zero_sum_row") else None)
    return ob, au


def digest(t, k=64):
    """tests/golden/make_golden.py's digest: element sum, absolute sum (float64), the first k values and k values at a fixed stride."""
    x = t.detach().double().reshape(-1).cpu()
    idx = torch.linspace(0, x.numel() - 1, k).long()
    return np.concatenate([[float(x.sum()), float(x.abs().sum())], x[:k].numpy(), x[idx].numpy()])


def model_case(g, tag, dtype=torch.float32, args_extra=None):
    """(model, batch, meta, args) of a stored case on the device: parameters by name, inputs by seed."""
    import bist_amd.model as M
    from bist_amd.data.batch import Batch
    meta = case_meta(g, tag)
    dm = meta["dims"]
    names = [(k, tuple(s)) for k, s in json.loads(str(g[f"{tag}_names"]))] if f"{tag}_names" in g.files else None
    args = cfg_args(meta["cfg"])
    for k, v in (args_extra or {}).items():
        setattr(args, k, v)
    model = M.make_model(dm["V"], dm["V"], args, ft_sizes=[dm["C"], dm["Da"]])
    if names is None:
        names = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd = audio_state(names)
    if meta.get("bf16_values"):
        sd = {k: v.bfloat16().float() for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    model = model.to("cuda").to(dtype).eval()
    ob, au = case_batch(meta)
    fts, au = ob.fts, torch.from_numpy(au)
    if meta.get("bf16_values"):
        fts, au = fts.bfloat16().float(), au.bfloat16().float()
    b = Batch(ob.query.cuda(), ob.his.cuda(), fts.cuda().to(dtype), ob.cap.cuda(), ob.trg.cuda(), ob.trg_y.cuda(),
              audio_fts=[au.cuda().to(dtype)])
    return model, b, meta, args
