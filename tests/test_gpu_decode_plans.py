"""smm_decode_f32 under every COMPOSITION of its plan features -- the stream split (choose_split, or the time-split videos as
the critical part), the time split of long videos, four-wave workgroups for the <= 16-state videos at the tail of a part -- on
one small launch of five parameter groups (tests/decode_corpus.py), plain and dressed (narration constraints, end penalties, a
class map, gaps on the frame axis).  The launch tags and the error words tell that a plan really had the features it was meant
to have; every output of every plan equals the baseline plan's bit for bit, from a freshly staged call and from a resident plan;
and the baseline is checked against the C twin.  (tests/test_decode_plans_host.py pins, on the host, what this leans on.)"""
import numpy as np
import pytest
import torch

import decode_corpus as DC

pytestmark = pytest.mark.gpu

SPLIT, NO_SPLIT = {'SMM_SPLIT_MIN_US': '0'}, {'SMM_NO_SPLIT': '1'}
CHUNK, NO_CHUNK = {'SMM_CHUNK': '1', 'SMM_CHUNK_P': '1'}, {'SMM_CHUNK': '0'}
SMALL, NO_SMALL = {'SMM_SMALL_WG': '2'}, {'SMM_SMALL_WG': '0'}
BASELINE = {**NO_SPLIT, **NO_CHUNK, **NO_SMALL}
# plan -> (switches, DP launch tags of one call, videos split in time)
PLANS = {
    'stream_split': ({**SPLIT, **NO_CHUNK, **NO_SMALL}, [1, 2], 0),
    'time_split': ({**NO_SPLIT, **CHUNK, **NO_SMALL}, [0], 3),
    'time_and_stream_split': ({**SPLIT, **CHUNK, **NO_SMALL}, [1, 2], 3),
    'small_tail': ({**NO_SPLIT, **NO_CHUNK, **SMALL}, [0, 3], 0),
    'stream_split_and_small_tail': ({**SPLIT, **NO_CHUNK, **SMALL}, [1, 2, 3], 0),
    'all_three': ({**SPLIT, **CHUNK, **SMALL}, [1, 2, 3], 3),
}
SWITCHES = ('SMM_NO_SPLIT', 'SMM_SPLIT_MIN_US', 'SMM_CHUNK', 'SMM_CHUNK_P', 'SMM_SMALL_WG', 'SMM_PLAN_CACHE', 'SMM_SPLIT_NS',
            'SMM_SPLIT_MARGIN', 'SMM_CHUNK_WC', 'SMM_CHUNK_LMIN')
KEYS = ('spans', 'labels', 'best', 'n_segs', 'elp')

_device = {}
_baseline = {}


def set_plan(monkeypatch, switches):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv(name, value)


def on_device(dressing):
    """The launch's inputs on the GPU, uploaded once per dressing: (batch, positional arguments of ops.decode, keyword ones)."""
    if dressing not in _device:
        cp = DC.corpus(dressing)
        dev = torch.device('cuda:0')
        t64 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
        args = (torch.tensor(cp['x'], device=dev), t64(cp['w']), t64(cp['cst']), t64(cp['inv_var']), t64(cp['trans']),
                t64(cp['init']), t64(cp['lens']))
        kw = dict(cons=None if cp['cons'] is None else torch.tensor(cp['cons'], device=dev), endpen=t64(cp['endpen']),
                  class_map=None if cp['class_map'] is None else torch.tensor(cp['class_map'], dtype=torch.int64, device=dev))
        _device[dressing] = (DC.make_batch(cp), args, kw)
    return _device[dressing]


def decode(dressing):
    """One ops.decode(..., want_elp=True) under the switches as they stand -> (outputs and error words on the host, the tags
    of the DP launches the call made)."""
    from action_segmentation_amd import ops
    batch, args, kw = on_device(dressing)
    ops.dp_timing_read()
    ops.dp_timing(True)
    try:
        out = ops.decode(batch, *args, want_elp=True, **kw)
        torch.cuda.synchronize()
    finally:
        ops.dp_timing(False)
    tags = sorted(t for _, t in ops.dp_timing_read(tagged=True))
    ops.check_decoded(batch, out)
    return {k: v.cpu().numpy() for k, v in out.items()}, tags


def baseline(dressing, monkeypatch):
    """The baseline plan's outputs (one DP launch on the caller's stream, no video split in time, eight-wave workgroups only),
    decoded once per dressing and kept."""
    if dressing not in _baseline:
        set_plan(monkeypatch, BASELINE)
        out, tags = decode(dressing)
        assert tags == [0], tags
        assert out['_err'][0] == 0 and out['_err'][4] == 0, out['_err']
        _baseline[dressing] = out
    return _baseline[dressing]


def assert_same_bits(out, base, what):
    for key in KEYS:
        np.testing.assert_array_equal(out[key], base[key], err_msg='%s: %s' % (what, key))


@pytest.mark.parametrize('dressing', DC.DRESSINGS)
def test_baseline_decode_equals_the_twin(dressing, monkeypatch):
    from action_segmentation_amd import ops
    cp, tw = DC.corpus(dressing), DC.twin(dressing)
    base = baseline(dressing, monkeypatch)
    set_plan(monkeypatch, BASELINE)
    batch, args, kw = on_device(dressing)
    b, lengths, off = cp['b'], cp['lengths'], cp['frame_off']
    # the two entry points one after the other: the same decode, bit for bit
    e64 = torch.zeros((cp['total'], DC.C_MAX), dtype=torch.float64, device=args[0].device)
    ops.emission(batch, *args[:4], cons=kw['cons'], out64=e64)
    two = ops.viterbi(batch, e64, *args[4:], endpen=kw['endpen'], class_map=kw['class_map'])
    torch.cuda.synchronize()
    ops.check_decoded(batch, two)
    for key in ('spans', 'labels', 'best', 'n_segs'):
        np.testing.assert_array_equal(two[key].cpu().numpy(), base[key], err_msg=key)
    # the emission: fp64 within test_emission_matches_oracle's tolerances of the direct form; the decode's fp32 copy is that, rounded
    e64 = e64.cpu().numpy()
    for i in range(b):
        c = DC.STATES[cp['group'][i]]
        np.testing.assert_allclose(e64[off[i]:off[i] + lengths[i], :c], tw['elp'][i], rtol=1e-12, atol=1e-9, err_msg='video %d' % i)
        np.testing.assert_allclose(base['elp'][off[i]:off[i] + lengths[i], :c], tw['elp'][i], rtol=2e-7, atol=1e-6, err_msg='video %d' % i)
    np.testing.assert_array_equal(base['elp'], e64.astype(np.float32))
    # the Viterbi kernels' standing claim, here with mixed groups, c_max padding, end penalties and the class map: the twin on
    # the GPU's own emission gives best and spans bit for bit
    own = [e64[off[i]:off[i] + lengths[i], :DC.STATES[cp['group'][i]]] for i in range(b)]
    spans, best = DC.twin_viterbi(cp, own)
    np.testing.assert_array_equal(base['best'], best)
    for i in range(b):
        t = int(lengths[i])
        np.testing.assert_array_equal(base['spans'][i, :t + 1], DC.global_ids(cp, i, spans[i]), err_msg='video %d' % i)
        assert (base['spans'][i, t + 1:] == -1).all()
        assert base['n_segs'][i] == (spans[i][:t] != -1).sum()
    # ... and on the REFERENCE emission: the same labels frame for frame (the corpus has no decision within the emission
    # kernel's rounding: test_decode_plans_host), EOS where each video ends, the score to rounding, -1 on frames no video covers
    np.testing.assert_allclose(base['best'], tw['best'], rtol=1e-12)
    for i in range(b):
        t, c = int(lengths[i]), DC.STATES[cp['group'][i]]
        np.testing.assert_array_equal(base['labels'][off[i]:off[i] + t], DC.global_ids(cp, i, tw['labels'][i]), err_msg='video %d' % i)
        assert base['spans'][i, t] == DC.global_ids(cp, i, c)
    assert (base['labels'][~DC.covered(cp)] == -1).all()
    assert (base['labels'][DC.covered(cp)] >= 0).all()


@pytest.mark.parametrize('plan', list(PLANS))
@pytest.mark.parametrize('dressing', DC.DRESSINGS)
def test_every_plan_decodes_to_the_baselines_bits(dressing, plan, monkeypatch):
    """Three calls under one plan: the first is staged into the workspace, the second sighting admits the resident plan, the
    third runs from it; then the same without resident plans.  Every call made the launches the plan is meant to make, and
    every output equals the baseline's."""
    from action_segmentation_amd import ops
    switches, want_tags, want_cut = PLANS[plan]
    base = baseline(dressing, monkeypatch)
    for cache in ('1', '0'):
        set_plan(monkeypatch, {**switches, 'SMM_PLAN_CACHE': cache})
        ops.release_cached_plans()                                 # (so that the first call below is this plan's first sighting)
        assert ops.cached_plan_bytes() == 0
        for call in range(3):
            out, tags = decode(dressing)
            what = '%s, SMM_PLAN_CACHE=%s, call %d' % (plan, cache, call)
            assert tags == want_tags, (what, tags)
            assert out['_err'][0] == 0 and out['_err'][4] == want_cut, (what, out['_err'])
            assert out['_err'][5] == 0, (what, out['_err'])         # a structured corpus: every cut certifies, nothing is decoded again
            assert_same_bits(out, base, what)
            # the resident plan: admitted at the second sighting, never without the cache
            assert (ops.cached_plan_bytes() > 0) == (cache == '1' and call >= 1), what
