"""Beam search with the audio modality (model/decode.py): the turn's static buffers stage audio_fts / audio_mask (audio length padded to
multiples of 32 with zero rows, masked by construction), audio_ft joins the per-turn reasoning cache, and under enc_vc_combine='dyn' the
persistent decoder launch and the device beam turn run unchanged (they attend encoded_ft only); under 'none' with audio the decoder layer
has a seventh attention and runs layer by layer.

Bounds: against the reference's n-best (g9_audio_wide.npz beam_*, weights and inputs bf16-representable on both sides) identical token
lists and scores within 8e-2, the bf16 bound of tests/test_model_gpu.py:486-488; a turn against the same turn on the layer-by-layer
decoder identical token lists and scores within 5e-2 (tests/test_model_gpu.py:374-376); fp32 against fp32 on another launch path within
1e-3 (tests/test_model_gpu.py:149)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_util as AU                                   # noqa: E402

from oracle import bist_oracle as O                       # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import bist_amd.model as M
    from bist_amd.data.batch import Batch
    return M, Batch


@pytest.fixture(scope="module")
def wide(hip, golden_dir):
    g = np.load(os.path.join(golden_dir, "g9_audio_wide.npz"))
    model, _, meta, args = AU.model_case(g, "wide", dtype=torch.bfloat16)
    return g, model, args


def _dialogue(hip, meta_dims, cfg, dtype, Ta=None, seed=None, audio_seed=None):
    M, Batch = hip
    dims = dict(meta_dims)
    if Ta is not None:
        dims.update(Ta=Ta, seed=seed, audio_seed=audio_seed)
    ob, au = AU.case_batch({"cfg": cfg, "dims": dims})
    fts, au = ob.fts.bfloat16().float(), torch.from_numpy(au).bfloat16().float()
    return Batch(ob.query.cuda(), ob.his.cuda(), fts.cuda().to(dtype), ob.cap.cuda(), ob.trg.cuda(), ob.trg_y.cuda(),
                 audio_fts=[au.cuda().to(dtype)])


def _turn(model, b, args, maxlen=12):
    from bist_amd.model.decode import beam_search_decode
    with torch.no_grad():
        return beam_search_decode(model, b, maxlen, O.SOS_ID, O.UNK_ID, O.EOS_ID, O.PAD_ID, beam=5, penalty=1.0, nbest=5, train_args=args)[0]


def _tokens(hyps):
    return [[int(t) for t in h[0]] for h in hyps]


def _drop(model):
    model.__dict__.pop("_bist_step_graphs", None); model.__dict__.pop("_bist_step_graphs_key", None)


def test_beam_search_reproduces_the_reference_n_best_on_the_device_beam_turn(hip, wide):
    import json
    import bist_amd.model.decode as D
    from bist_amd import _lib
    g, model, args = wide
    meta = json.loads(str(g["beam_cfg"]))
    b = _dialogue(hip, meta["dims"], meta["cfg"], torch.bfloat16)
    assert tuple(b.audio_fts.shape) == (1, 24, 128)
    _drop(model)
    before = dict(D.STATS)
    _lib.lib.bist_launch_count_reset()
    for _ in range(2):                       # the second turn replays the captured graphs
        hyps = _turn(model, b, args)
    assert D.STATS["device"] - before["device"] == 2 and D.STATS["host"] == before["host"], (before, D.STATS)
    assert _lib.lib.bist_launch_count(_lib.K_DECSTACK) >= 12
    assert len(hyps) == int(g["beam_n"])
    for i, (toks, score) in enumerate(hyps):
        print("hyp", i, [int(t) for t in toks], float(score), float(g[f"beam_score{i}"]))
    for i, (toks, score) in enumerate(hyps):
        assert [int(t) for t in toks] == g[f"beam_hyp{i}"].tolist(), (i, toks)
        assert abs(float(score) - float(g[f"beam_score{i}"])) <= 8e-2, (i, float(score), float(g[f"beam_score{i}"]))


def test_turns_of_different_audio_lengths_reuse_the_step_graphs_and_share_no_state(hip, wide):
    """Audio lengths 24, then 40, then 50: the static buffers hold 32, 64 and 64 audio rows.  The step graphs (one per step of the
    beam) do not depend on the audio length and are captured once; the first-step graph is per padded audio length: the second turn
    captures exactly that one, the third nothing.  Every turn equals the same turn on the layer-by-layer decoder with full-prefix steps."""
    import json
    import bist_amd.model.decode as D
    from bist_amd import functional as Fn
    g, model, args = wide
    meta = json.loads(str(g["beam_cfg"]))
    turns = [_dialogue(hip, meta["dims"], meta["cfg"], torch.bfloat16, Ta=ta, seed=500 + ta, audio_seed=600 + ta) for ta in (24, 40, 50)]
    _drop(model)
    fast, captures = [], []
    for b in turns:
        c0 = D.STATS["captures"]
        fast.append(_turn(model, b, args))
        captures.append(D.STATS["captures"] - c0)
    again = _turn(model, turns[0], args)
    assert captures[0] >= 12 and captures[1] == 1 and captures[2] == 0, captures
    store = model.__dict__["_bist_step_graphs"]
    firsts = [k for k in store if isinstance(k, tuple) and k and k[0] == "first"]
    assert len(firsts) == 2
    staged = sorted(dict((f, s) for f, s in k[1:])["audio_fts"][0][1] for k in firsts)
    assert staged == [32, 64]
    Fn.FUSED_DECODE, D.INCREMENTAL = False, False
    _drop(model)
    try:
        slow = [_turn(model, b, args) for b in turns]
    finally:
        Fn.FUSED_DECODE, D.INCREMENTAL = True, True
        _drop(model)
    for i, (a, c) in enumerate(zip(fast, slow)):
        assert _tokens(a) == _tokens(c), i
        assert max(abs(float(x[1]) - float(y[1])) for x, y in zip(a, c)) <= 5e-2, i
    assert _tokens(again) == _tokens(fast[0])
    assert _tokens(fast[1]) != _tokens(fast[0]) or _tokens(fast[2]) != _tokens(fast[1])          # (different dialogues: the turns are not copies)


def test_none_mode_with_audio_runs_the_layer_by_layer_decoder(hip, golden_dir):
    """enc_vc_combine='none' with audio: seven attentions per decoder layer, so the persistent launch (four) must not be used; the
    graph-replayed turn equals the turn decoded with plain model.encode / model.decode calls."""
    import bist_amd.model.decode as D
    from bist_amd import _lib
    g = np.load(os.path.join(golden_dir, "g9_audio_none.npz"))
    model, b4, meta, args = AU.model_case(g, "none")
    M, Batch = hip
    ob, au = AU.case_batch(meta)
    b = Batch(ob.query[:1].cuda(), ob.his[:1].cuda(), ob.fts[:1].cuda(), ob.cap[:1].cuda(), ob.trg[:1].cuda(), ob.trg_y[:1].cuda(),
              audio_fts=[torch.from_numpy(au[:1]).cuda()])
    dec = model.mutlimodal_decoder
    with torch.no_grad():
        ft = model.encode(b)
        assert not dec._fused_decode_ok(b, dict(ft, _bist_shared_rows=True), ft["encoded_query"][:, :1])
    _drop(model)
    _lib.lib.bist_launch_count_reset()
    before = dict(D.STATS)
    fast = _turn(model, b, args, maxlen=8)
    assert _lib.lib.bist_launch_count(_lib.K_DECSTACK) == 0 and D.STATS["device"] == before["device"]
    assert "audio_ft" in dec._REASONING_KEYS
    D.STEP_GRAPHS = False
    _drop(model)
    try:
        slow = _turn(model, b, args, maxlen=8)
    finally:
        D.STEP_GRAPHS = True
    assert len(fast) == len(slow) and len(fast) > 1
    assert _tokens(fast) == _tokens(slow)
    assert max(abs(float(x[1]) - float(y[1])) for x, y in zip(fast, slow)) <= 1e-3
