#!/usr/bin/env python3
"""Generate the AUDIO golden vectors (g9_*) by RUNNING THE REFERENCE with its audio stack on.

Like make_golden.py this runs only where the reference checkout exists (never on the GPU machine) and imports the reference's own
modules unmodified, with the same capture-process shims (the ``nltk`` stub, ``.cuda()`` as identity).  One more thing is needed: the
reference's audio branch reads ``args.noW_venc`` (model/encoder.py:84), which no config defines, so the Namespace handed to
``make_model`` carries ``noW_venc=False``.

The CPU oracle does not model audio, so there is no ``det_state`` for these models: the file stores the reference model's own
``state_dict()`` names and shapes, and the tests regenerate every parameter as ``O.det_param(name, shape)`` (tests/audio_util.py:
``audio_state``).  The audio input is regenerated from the seed stored with each case (``audio_input``).

Files (each below 1 MiB):
  g9_audio.npz              small-dyn, small-nocap, zero-sum row, long audio (fp32 tensors), the pickled module's outputs
  g9_audio_wide.npz         wide (digests of every ft tensor, log-probs and gradient; loss terms) and the beam search on its model
  g9_audio_none.npz         small-none: log-probs, loss terms, gradients of the decoder layers' seven attentions
  g9_audio_module.pth.tar   ``torch.save(model)`` of a tiny audio model by the reference (whole-module pickle, as g7), with its
                            log-probs in g9_audio.npz under "module_*".  (The small-dyn model itself would be a 2.6 MB pickle.)

usage:  python tests/golden/make_golden_audio.py      (from the repository root)
"""
import argparse
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BIST_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

sys.modules.setdefault("nltk", types.ModuleType("nltk"))
sys.modules.setdefault("nltk.util", types.ModuleType("nltk.util"))
sys.modules["nltk.util"].ngrams = lambda *a, **k: None
torch.Tensor.cuda = lambda self, *a, **k: self

from oracle import bist_oracle as O          # noqa: E402  (det_param / det_batch / Cfg only)
import audio_util as AU                       # noqa: E402
import model.mtn as R                         # noqa: E402  the reference
import model.decode as RD                     # noqa: E402
from model.label_smoothing import LabelSmoothing   # noqa: E402
from model.optimize import SimpleLossCompute       # noqa: E402
from data.dataset import Batch as RBatch      # noqa: E402

SMALL = dict(B=2, T=6, S=9, C=48, Lq=7, Lh=11, Lc=8, Lt=6, V=60)        # make_golden.py's SMALL
MID = dict(B=2, T=8, S=49, C=64, Lq=20, Lh=24, Lc=12, Lt=10, V=120)


def npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def ref_args(cfg):
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model, "noW_venc": False})


def build(cfg, dims, bf16_values=False):
    """The reference model with deterministic parameters by name -> (model, [(name, shape)])."""
    model = R.make_model(dims["V"], dims["V"], ref_args(cfg), ft_sizes=[dims["C"], dims["Da"]])
    names = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.endswith(".pe")]
    sd = AU.audio_state(names)
    if bf16_values:
        sd = {k: v.bfloat16().float() for k, v in sd.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    assert model.generator.vocab_gen is model.query_embed[0].lut.weight
    model.eval()
    return model, names


def ref_batch(ob, au):
    return RBatch(ob.query, ob.his, [ob.fts.numpy()], ob.cap, ob.trg, ob.trg_y, O.PAD_ID, None, None, audio_fts=[au])


def loss_terms(model, cfg, ft, rb, vocab):
    """Each term exactly as optimize.py:46-83 forms it, in its order: out, cap_ae, audio_ae, temporal_ae, spatial_ae."""
    crit = LabelSmoothing(size=vocab, padding_idx=O.PAD_ID, smoothing=0.1)
    args = ref_args(cfg)
    logp = model.generator(ft, rb, args)
    norm, qn = rb.ntokens.float(), rb.qntokens.float()
    terms = {"out": crit(logp.contiguous().view(-1, vocab), rb.trg_y.contiguous().view(-1)) / norm}
    if cfg.auto_encoder:
        pairs = []
        if cfg.nb_cenc_blocks > 0:
            pairs.append(("cap_ae", "cap_ft"))
        if cfg.nb_aenc_blocks > 0:
            pairs.append(("audio_ae", "audio_ft"))
        if cfg.nb_venc_blocks > 0 and cfg.s2t:
            pairs.append(("temporal_ae", "temporal_ft"))
        if cfg.nb_venc_blocks > 0 and cfg.t2s:
            pairs.append(("spatial_ae", "spatial_ft"))
        for name, key in pairs:
            lp = model.ae_generator(ft, rb, args, key)
            terms[name] = crit(lp.contiguous().view(-1, vocab), rb.query.contiguous().view(-1)) / qn
    total = sum(terms.values())
    rep = SimpleLossCompute(model.generator, model.ae_generator, crit, opt=None, args=args)(ft, rb)
    assert abs(float(rep["out"]) - float(terms["out"] * norm)) < 1e-2 * max(1.0, abs(float(rep["out"])))
    return logp, terms, total


def case_small(tag, cfg, dims, out, store_ft=(), grads=None, with_grad=False):
    """Forward, log-probs, loss terms (and gradients of the parameters `grads` selects by name) through the reference."""
    model, names = build(cfg, dims)
    meta = {"cfg": cfg.__dict__, "dims": dims}
    ob, au = AU.case_batch(meta)
    rb = ref_batch(ob, au)
    assert torch.equal(rb.audio_mask, (torch.from_numpy(au).sum(-1) != 0).unsqueeze(-2))
    with (torch.enable_grad() if with_grad else torch.no_grad()):
        ft = model.forward(rb)
        logp, terms, total = loss_terms(model, cfg, ft, rb, dims["V"])
        if with_grad:
            total.backward()
    for k in (ft if store_ft == "all" else store_ft):
        out[f"{tag}_ft_{k}"] = npy(ft[k])
    out[f"{tag}_audio_mask"] = npy(rb.audio_mask)
    out[f"{tag}_logp"] = npy(logp)
    for k, v in terms.items():
        out[f"{tag}_loss_{k}"] = npy(v)
    out[f"{tag}_loss_total"] = npy(total)
    if with_grad:
        for k, p in model.named_parameters():
            if grads(k):
                out[f"{tag}_grad_{k}"] = npy(p.grad)
    out[f"{tag}_cfg"] = np.asarray(json.dumps(meta))
    out[f"{tag}_names"] = np.asarray(json.dumps(names))
    return model


def case_wide(out):
    """d_model = 512: the bf16 production kernels' geometry.  Weights and inputs are rounded to bf16 BEFORE the reference runs (as
    tests/test_production_gpu.py does for the oracle), so the digests measure the path's arithmetic, not the rounding of its inputs."""
    cfg = O.Cfg(d_model=512, att_h=8, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2, nb_aenc_blocks=2)
    dims = dict(MID, Ta=24, Da=128, audio_seed=909, seed=4243)
    model, names = build(cfg, dims, bf16_values=True)
    meta = {"cfg": cfg.__dict__, "dims": dims, "bf16_values": True}
    ob, au = AU.case_batch(meta)
    ob.fts = ob.fts.bfloat16().float()
    au = torch.from_numpy(au).bfloat16().float().numpy()
    rb = ref_batch(ob, au)
    ft = model.forward(rb)
    logp, terms, total = loss_terms(model, cfg, ft, rb, dims["V"])
    total.backward()
    for k, v in ft.items():
        out[f"wide_dg_{k}"] = AU.digest(v)
    out["wide_dg_logp"] = AU.digest(logp)
    out["wide_argmax"] = npy(logp.argmax(-1))
    for k, v in terms.items():
        out[f"wide_loss_{k}"] = npy(v)
    for k, p in model.named_parameters():
        if p.grad is None:                        # (parameters no output depends on)
            print("no gradient:", k)
            continue
        out[f"wide_gdg_{k}"] = AU.digest(p.grad)
        out[f"wide_gmax_{k}"] = np.asarray(float(p.grad.abs().max()))
    out["wide_cfg"] = np.asarray(json.dumps(meta))
    out["wide_names"] = np.asarray(json.dumps(names))
    # beam search on one dialogue with the same model
    bdims = dict(dims, B=1, seed=4244, audio_seed=910, zero_tail=[], maxlen=12, beam=5, nbest=5)
    bmeta = {"cfg": cfg.__dict__, "dims": bdims, "bf16_values": True}
    ob1, au1 = AU.case_batch(bmeta)
    ob1.fts = ob1.fts.bfloat16().float()
    au1 = torch.from_numpy(au1).bfloat16().float().numpy()
    with torch.no_grad():
        hyps, best = RD.beam_search_decode(model, ref_batch(ob1, au1), 12, O.SOS_ID, O.UNK_ID, O.EOS_ID, O.PAD_ID, beam=5, penalty=1.0,
                                           nbest=5, train_args=ref_args(cfg))
    out["beam_n"] = np.asarray(len(hyps))
    for i, (toks, score) in enumerate(hyps):
        out[f"beam_hyp{i}"] = np.asarray([int(t) for t in toks], dtype=np.int64)
        out[f"beam_score{i}"] = np.asarray(float(score))
    out["beam_cfg"] = np.asarray(json.dumps(bmeta))


def case_module(out):
    """A whole-module pickle written by the reference (train.py:161) for a tiny audio model, with its outputs."""
    cfg = O.Cfg(d_model=16, att_h=2, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1, nb_aenc_blocks=1)
    dims = dict(B=2, T=4, S=9, C=8, Lq=5, Lh=6, Lc=4, Lt=5, V=30, seed=5, Ta=5, Da=8, audio_seed=911, zero_tail=[[1, 2]])
    model, names = build(cfg, dims)
    torch.save(model, os.path.join(HERE, "g9_audio_module.pth.tar"))
    meta = {"cfg": cfg.__dict__, "dims": dims}
    ob, au = AU.case_batch(meta)
    rb = ref_batch(ob, au)
    with torch.no_grad():
        ft = model.forward(rb)
        out["module_logp"] = npy(model.generator(ft, rb, ref_args(cfg)))
    out["module_ft_encoded_audio"] = npy(ft["encoded_audio"])
    out["module_ft_encoded_ft"] = npy(ft["encoded_ft"])
    out["module_cfg"] = np.asarray(json.dumps(meta))
    out["module_names"] = np.asarray(json.dumps(names))


def main():
    small = dict(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2, nb_aenc_blocks=2)
    dims = dict(SMALL, Ta=9, Da=16, audio_seed=901)
    audio_param = lambda k: any(s in k for s in ("vid_encoder.a_W", "vid_encoder.a_in_norm", ".a_layers.", ".a_out_norm."))
    out = {}
    case_small("dyn", O.Cfg(**small), dims, out, store_ft="all", with_grad=True,
               grads=lambda k: audio_param(k) or "vc_combine_W" in k or k == AU.LUT)
    case_small("nocap", O.Cfg(**dict(small, nb_cenc_blocks=0, include_caption="none")), dims, out, store_ft=("encoded_ft",))
    case_small("zerosum", O.Cfg(**small), dict(dims, zero_sum_row=[0, 2]), out)
    case_small("long", O.Cfg(**small), dict(dims, Ta=70, audio_seed=902), out, with_grad=True, grads=lambda k: k.startswith("vid_encoder.a_W"))
    case_module(out)
    np.savez_compressed(os.path.join(HERE, "g9_audio.npz"), **out)
    out = {}
    case_wide(out)
    np.savez_compressed(os.path.join(HERE, "g9_audio_wide.npz"), **out)
    out = {}
    case_small("none", O.Cfg(**dict(small, enc_vc_combine="none")), dims, out, with_grad=True,
               grads=lambda k: ".layers." in k and ".attn." in k)
    np.savez_compressed(os.path.join(HERE, "g9_audio_none.npz"), **out)
    for f in ("g9_audio.npz", "g9_audio_wide.npz", "g9_audio_none.npz", "g9_audio_module.pth.tar"):
        print(f, os.path.getsize(os.path.join(HERE, f)) // 1024, "KiB")


if __name__ == "__main__":
    main()
