"""The audio modality's host side (reference: model/mtn.py:110-147, model/encoder.py:55-93, data/dataset.py:83-87, model/optimize.py:61-65):
construction and state_dict names against the reference's own list (tests/golden/g9_audio.npz), the Batch mask rule, the audio length
class, the loss terms' order, the missing ``noW_venc``, and the reference's whole-module pickle of an audio model.  No GPU."""
import argparse
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_util as AU                                   # noqa: E402

from bist_amd.data.classes import DEFAULT_AUDIO_RUNGS, DEFAULT_AUDIO_STEP, FIELDS, LengthClasses      # noqa: E402


@pytest.fixture(scope="module")
def g9(golden_dir):
    return np.load(os.path.join(golden_dir, "g9_audio.npz"))


def _names(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.endswith(".pe")]


@pytest.mark.parametrize("tag", ["dyn", "nocap", "module"])
def test_make_model_with_audio_builds_with_the_reference_names_and_shapes(g9, tag):
    """make_model(..., ft_sizes=[C, Da]) with nb_aenc_blocks = 2: vid_encoder.a_W / a_in_norm, mutlimodal_decoder.a_layers.N / a_out_norm,
    vc_combine_W sized by the reference's factor ([4, 5d] with a caption stack, [3, 4d] without)."""
    import bist_amd.model as M
    meta = AU.case_meta(g9, tag)
    dm = meta["dims"]
    model = M.make_model(dm["V"], dm["V"], AU.cfg_args(meta["cfg"]), ft_sizes=[dm["C"], dm["Da"]])
    want = [(k, tuple(s)) for k, s in json.loads(str(g9[f"{tag}_names"]))]
    assert sorted(_names(model)) == sorted(want)
    d = meta["cfg"]["d_model"]
    n = 5 if meta["cfg"]["nb_cenc_blocks"] > 0 else 4
    assert tuple(model.mutlimodal_decoder.vc_combine_W.weight.shape) == (n - 1, n * d)
    assert len(model.mutlimodal_decoder.a_layers) == meta["cfg"]["nb_aenc_blocks"]
    missing, unexpected = model.load_state_dict(AU.audio_state(want), strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)


def test_none_mode_gives_the_decoder_layer_a_seventh_attention(golden_dir):
    import bist_amd.model as M
    g = np.load(os.path.join(golden_dir, "g9_audio_none.npz"))
    meta = AU.case_meta(g, "none")
    dm = meta["dims"]
    model = M.make_model(dm["V"], dm["V"], AU.cfg_args(meta["cfg"]), ft_sizes=[dm["C"], dm["Da"]])
    assert len(model.mutlimodal_decoder.layers[0].attn) == 7 and len(model.mutlimodal_decoder.layers[0].sublayer) == 8
    assert not hasattr(model.mutlimodal_decoder, "vc_combine_W")
    assert sorted(_names(model)) == sorted((k, tuple(s)) for k, s in json.loads(str(g["none_names"])))


def test_audio_layers_need_the_audio_width():
    import bist_amd.model as M
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=16, att_h=2, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1, nb_aenc_blocks=1)
    with pytest.raises(ValueError):
        M.make_model(30, 30, AU.cfg_args(cfg.__dict__), ft_sizes=[8])


def test_audio_with_one_visual_direction_is_refused_at_construction():
    """decoder.py:160-167 indexes score column 3 of three: the reference cannot run it, so the model does not build ('none' does)."""
    import bist_amd.model as M
    from oracle import bist_oracle as O
    for kw in (dict(s2t=0), dict(t2s=0), dict(s2t=0, nb_cenc_blocks=0, include_caption="none")):
        cfg = O.Cfg(**{**dict(d_model=16, att_h=2, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1, nb_aenc_blocks=1), **kw})
        with pytest.raises(NotImplementedError, match="one visual direction"):
            M.make_model(30, 30, AU.cfg_args(cfg.__dict__), ft_sizes=[8, 4])
    cfg = O.Cfg(d_model=16, att_h=2, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1, nb_aenc_blocks=1, s2t=0, enc_vc_combine="none")
    assert len(M.make_model(30, 30, AU.cfg_args(cfg.__dict__), ft_sizes=[8, 4]).mutlimodal_decoder.a_layers) == 1


def test_batch_masks_audio_rows_by_their_sum(g9):
    """audio_mask = (audio_fts.sum(-1) != 0).unsqueeze(-2): all-zero rows AND a row of +1, -1, 0, ... are masked (dataset.py:87);
    audio_fts is taken as the reference passes it: a list holding one array."""
    from bist_amd.data.batch import Batch, SourceBatch
    for tag in ("dyn", "zerosum"):
        meta = AU.case_meta(g9, tag)
        ob, au = AU.case_batch(meta)
        b = Batch(ob.query, ob.his, ob.fts, ob.cap, ob.trg, ob.trg_y, audio_fts=[au])
        assert b.audio_fts.dtype == torch.float32 and tuple(b.audio_fts.shape) == (meta["dims"]["B"], meta["dims"]["Ta"], meta["dims"]["Da"])
        assert b.audio_mask.dtype == torch.bool and tuple(b.audio_mask.shape) == (meta["dims"]["B"], 1, meta["dims"]["Ta"])
        assert np.array_equal(b.audio_mask.numpy(), g9[f"{tag}_audio_mask"])
        s = SourceBatch(ob.query, ob.his, ob.fts, ob.cap, ob.trg, ob.trg_y, audio_fts=torch.from_numpy(au))
        assert "audio_mask" not in s.__dict__ and torch.equal(s.audio_mask, b.audio_mask)
    m = g9["zerosum_audio_mask"]
    assert not m[0, 0, 2] and m[0, 0, 1] and not m[1, 0, -3:].any()            # the zero-sum row, a live row, clip 1's zero tail
    none = Batch(ob.query, ob.his, ob.fts, ob.cap, ob.trg, ob.trg_y)
    assert none.audio_fts is None and none.audio_mask is None
    assert Batch(ob.query, ob.his, ob.fts, ob.cap, ob.trg, ob.trg_y, audio_fts=[]).audio_fts is None


class _B:
    def __init__(self, B=4, Lq=7, Lh=9, Lc=6, Lt=6, T=6, S=9, C=64, cap=True, dtype=torch.float32, audio=None):
        self.query = torch.zeros(B, Lq, dtype=torch.int64)
        self.his = torch.zeros(B, Lh, dtype=torch.int64)
        self.cap = torch.zeros(B, Lc, dtype=torch.int64) if cap else None
        self.trg = torch.zeros(B, Lt, dtype=torch.int64)
        self.trg_y = torch.zeros(B, Lt, dtype=torch.int64)
        self.fts = torch.zeros(B, T, S, C, dtype=dtype)
        self.audio_fts = torch.zeros(B, audio[0], audio[1], dtype=dtype) if audio else None


def test_length_classes_without_audio_are_what_they_were():
    """Literal key() / shape() of two batches, recorded from the commit before audio (its bist_amd/data/classes.py, same inputs)."""
    lc = LengthClasses()
    assert FIELDS == ("query", "his", "cap", "trg", "frames")
    a = _B(Lq=20, Lh=60, Lc=25, Lt=20, T=32)
    assert lc.key(a) == (4, 24, 64, 32, 24, 32, (9, 64), "torch.float32", "torch.int64", True, True)
    assert lc.shape(a) == {"query": 24, "his": 64, "cap": 32, "trg": 24, "frames": 32}
    assert LengthClasses.lengths(a) == {"query": 20, "his": 60, "cap": 25, "trg": 20, "frames": 32}
    b = _B(B=3, Lq=33, Lh=300, Lt=7, T=63, S=49, C=2048, cap=False, dtype=torch.bfloat16)
    assert lc.key(b) == (3, 48, 320, None, 8, 63, (49, 2048), "torch.bfloat16", "torch.int64", False, True)
    assert lc.shape(b) == {"query": 48, "his": 320, "cap": None, "trg": 8, "frames": 63}
    assert list(lc.shape(b)) == list(FIELDS)


def test_length_classes_with_audio_grow_by_the_audio_rung():
    lc = LengthClasses()
    plain = _B(Lq=20, Lh=60, Lc=25, Lt=20, T=32)
    for Ta, rung in ((1, 16), (9, 16), (16, 16), (20, 32), (33, 48), (64, 64), (65, 96), (70, 96), (129, 160)):
        b = _B(Lq=20, Lh=60, Lc=25, Lt=20, T=32, audio=(Ta, 128))
        assert lc.shape(b) == dict(lc.shape(plain), audio=rung), Ta
        assert lc.key(b)[:len(lc.key(plain))] == lc.key(plain) and lc.key(b)[len(lc.key(plain))] == rung, Ta
    assert lc.key(_B(audio=(9, 128))) == lc.key(_B(audio=(16, 128))) != lc.key(_B(audio=(17, 128)))
    assert lc.key(_B(audio=(9, 128))) != lc.key(_B(audio=(9, 16)))              # the feature width shapes the graph
    one = LengthClasses.fixed(query=32, his=128, cap=64, trg=32, frames=32, audio=64)
    assert len({one.key(_B(audio=(Ta, 128))) for Ta in (1, 9, 33, 64)}) == 1


def test_default_audio_rungs_do_not_straddle_64():
    """The small-attention MFMA backward covers Lk <= 64 keys: a class must select the kernel form of every exact length mapped to it."""
    assert DEFAULT_AUDIO_RUNGS == (16, 32, 48, 64) and DEFAULT_AUDIO_STEP == 32
    lc = LengthClasses()
    for Ta in range(1, 400):
        P = lc.round("audio", Ta)
        assert P >= Ta and (Ta <= 64) == (P <= 64), (Ta, P)
        assert P in DEFAULT_AUDIO_RUNGS or P % 32 == 0


def test_term_names_put_audio_ae_where_the_reference_adds_it():
    """optimize.py:55-82: out, cap_ae, audio_ae, temporal_ae, spatial_ae."""
    from bist_amd.train import Trainer
    from oracle import bist_oracle as O
    base = dict(O.Cfg(nb_aenc_blocks=2).__dict__)
    names = lambda **kw: Trainer._term_names(types.SimpleNamespace(args=argparse.Namespace(**{**base, **kw})))
    assert names() == ["out", "cap_ae", "audio_ae", "temporal_ae", "spatial_ae"]
    assert names(nb_cenc_blocks=0) == ["out", "audio_ae", "temporal_ae", "spatial_ae"]
    assert names(nb_aenc_blocks=0) == ["out", "cap_ae", "temporal_ae", "spatial_ae"]
    assert names(auto_encoder=0) == ["out"]


def test_a_missing_noW_venc_counts_as_false(monkeypatch):
    """The reference reads args.noW_venc, which no config defines (encoder.py:84).  Here an absent attribute and False take the same
    branch -- the projection a_W -- and True skips it.  The launches are replaced by recorders: which branch ran is a host decision."""
    import bist_amd.model.encoder as E
    calls = []
    monkeypatch.setattr(E.Fn, "linear", lambda x, w, b=None, **kw: calls.append("a_W") or torch.zeros(x.shape[0], w.shape[0]))
    monkeypatch.setattr(E.LayerNorm, "forward", lambda self, x: x)
    W, aW = torch.nn.Linear(8, 16), torch.nn.Linear(4, 16)
    b = types.SimpleNamespace(fts=None, audio_fts=torch.ones(2, 3, 4))
    for ns, want in ((argparse.Namespace(), ["a_W"]), (argparse.Namespace(noW_venc=False), ["a_W"])):
        calls.clear()
        ft = E.VidEncoder8(W, aW, None, 0, 1, 16, ns)(b, {})
        assert calls == want and tuple(ft["encoded_audio"].shape) == (2, 3, 16)
    calls.clear()
    b16 = types.SimpleNamespace(fts=None, audio_fts=torch.ones(2, 3, 16))
    ft = E.VidEncoder8(W, aW, None, 0, 1, 16, argparse.Namespace(noW_venc=True))(b16, {})
    assert calls == [] and torch.equal(ft["encoded_audio"], b16.audio_fts)


def test_reference_audio_pickle_loads_through_the_model_mapping(g9, golden_dir):
    """a whole-module pickle WRITTEN BY THE REFERENCE for a model with the audio stack, unpickled by its
    ``model.*`` class paths into this build's classes."""
    import bist_amd.model as m
    names = ("", ".mtn", ".modules", ".encoder", ".decoder", ".generator", ".label_smoothing", ".optimize", ".decode")
    saved = {("model" + n): sys.modules.get("model" + n) for n in names}
    try:
        for n in names:
            sys.modules["model" + n] = sys.modules["bist_amd.model" + n] if n else m
        obj = torch.load(os.path.join(golden_dir, "g9_audio_module.pth.tar"), weights_only=False)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert type(obj) is m.mtn.MTN
    dec = obj.mutlimodal_decoder
    assert type(dec.a_layers[0]) is m.encoder.AudioEncoderLayer and type(obj.vid_encoder) is m.encoder.VidEncoder8
    assert dec.a_N == 1 and obj.vid_encoder.a_N == 1 and obj.args.noW_venc is False
    meta = AU.case_meta(g9, "module")
    assert tuple(obj.vid_encoder.a_W.weight.shape) == (meta["cfg"]["d_model"], meta["dims"]["Da"])
    want = AU.audio_state([(k, tuple(s)) for k, s in json.loads(str(g9["module_names"]))])
    got = obj.state_dict()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert obj.generator.vocab_gen is obj.query_embed[0].lut.weight
