"""Closed-form supervised fit on the device (csrc/smm_fit.hip) against the CPU restatement (oracle/dense_ref.py), which
is itself pinned to the reference's fit_supervised outputs (tests/golden, test_oracle_golden.py).
Integer statistics: exact.  Floating-point sums: fp64 with an unspecified addition order -> rel 1e-12.
The shapes cross every work split of the two kernels; the inputs that need a premise are in tests/fit_cases.py."""
import numpy as np
import pytest
import torch

import fit_cases as F
from oracle import dense_ref as O

pytestmark = pytest.mark.gpu


def make_videos(rng, n_videos, t_lo, t_hi, n_classes, d, mean_len, classes=None):
    feats, labels = [], []
    classes = list(range(n_classes)) if classes is None else classes
    for _ in range(n_videos):
        t = int(rng.integers(t_lo, t_hi + 1))
        y = []
        while len(y) < t:
            y += [int(rng.choice(classes))] * int(max(1, rng.poisson(mean_len)))
        y = np.asarray(y[:t], dtype=np.int64)
        x = (rng.normal(size=(t, d)) + y[:, None] * 0.1).astype(np.float32)
        feats.append(x)
        labels.append(y)
    return feats, labels


INT_KEYS = ('span_counts', 'span_lengths', 'span_start_counts', 'span_transition_counts')


def device_stats(feats, labels, n_classes, max_k):
    from action_segmentation_amd.semimarkov_utils import semimarkov_sufficient_stats_device
    return semimarkov_sufficient_stats_device([torch.from_numpy(f) for f in feats], [torch.from_numpy(l) for l in labels],
                                              'tied_diag', n_classes, max_k)


def assert_stats_match_oracle(feats, labels, n_classes, max_k, want=None):
    em, st = device_stats(feats, labels, n_classes, max_k)
    want = O.sufficient_stats(feats, labels, n_classes, max_k) if want is None else want
    for key in INT_KEYS:
        np.testing.assert_array_equal(st[key], want[key], err_msg=key)
    assert st['instance_count'] == want['instance_count']
    np.testing.assert_allclose(em.means_, want['means'], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(em.covariances_[0], want['var'], rtol=1e-11, atol=0)
    return em, st


@pytest.mark.parametrize('d,n_classes,max_k,t_hi', [(200, 9, 20, 700), (200, 9, 4, 300), (7, 5, 3, 90), (16, 40, 64, 2500),
                                                     (300, 6, None, 400), (1, 3, 2, 50)])
def test_sufficient_stats_match_oracle(d, n_classes, max_k, t_hi):
    rng = np.random.default_rng(d * 31 + n_classes)
    feats, labels = make_videos(rng, 7, 1, t_hi, n_classes, d, mean_len=11,
                                classes=[c for c in range(n_classes) if c != 2])     # class 2 never occurs
    em, _ = assert_stats_match_oracle(feats, labels, n_classes, max_k)
    assert np.all(em.means_[2] == 0)


@pytest.mark.parametrize('max_k', F.MAX_KS)
def test_span_stats_carry_the_open_run_across_chunks(max_k):
    """smm_span_stats_kernel's 2048-frame chunks: the start of the run that is open at a chunk's first frame decides where
    that run is cut once it has crossed the boundary.  Four videos (tests/fit_cases.py: CARRY_RUNS) put that start in the
    second trip of the 256-label backward scan, at frame 0 (the scan's p == 0 exit, through a chunk without a change), at
    c_begin - 1 (first lane of the first trip), on the first and second frame of the second trip, and a label change
    exactly on a boundary.  test_fit_cases_host.py shows on the CPU that a carry of 0 or of c_begin - 1 in place of the
    true start changes the span and transition counts at max_k = 20, 64 and 1025; None and 2 are the control."""
    feats, labels = F.carry_batch()
    assert_stats_match_oracle(feats, labels, F.N_CLASSES, max_k)


@pytest.fixture(scope='module')
def many_items_oracle():
    cache = {}

    def get(d):
        if d not in cache:
            feats = F.many_items_features(d)
            cache[d] = (feats, O.sufficient_stats(feats, F.many_items_labels(), F.MANY_CLASSES, F.MANY_MAX_K))
        return cache[d]
    return get


@pytest.mark.parametrize('d', [8, 6])
def test_class_sums_many_items_per_workgroup(many_items_oracle, d):
    """smm_class_sums_kernel with more work items than workgroups (tests/fit_cases.py: many_items_labels; 4008 items on a
    grid of 768): every workgroup walks its `item += gridDim.x` loop five or six times with the sum of squares kept in
    registers across the items, and most items lie past the end of their (short) video -- the `continue` in front of a
    live item.  D = 8: float4 path, D = 6: element-wise.  Integer statistics are the same on every run."""
    feats, want = many_items_oracle(d)
    labels = F.many_items_labels()
    em, st = assert_stats_match_oracle(feats, labels, F.MANY_CLASSES, F.MANY_MAX_K, want=want)
    assert np.all(em.means_[F.MANY_ABSENT] == 0)
    _, again = device_stats(feats, labels, F.MANY_CLASSES, F.MANY_MAX_K)
    for key in INT_KEYS:
        np.testing.assert_array_equal(again[key], st[key], err_msg=key)


@pytest.mark.parametrize('d', [256, 257, 260, 513, 516])
def test_class_sums_column_passes(d):
    """The 256-column passes of smm_class_sums_kernel: one pass of exactly 256 columns; a second pass of one column
    (element-wise) and of four (one float4 lane); a third pass of one column behind two full ones (513, element-wise) and of
    four (516, float4)."""
    n_classes = 6
    rng = np.random.default_rng(d)
    feats, labels = make_videos(rng, 3, 100, 300, n_classes, d, mean_len=11, classes=[c for c in range(n_classes) if c != 2])
    em, _ = assert_stats_match_oracle(feats, labels, n_classes, 20)
    assert np.all(em.means_[2] == 0)


def test_fit_supervised_on_device_matches_host_module_and_oracle():
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=2)
    host = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    host.fit(data, use_labels=True)
    dev = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=True, batch_size=2), data)
    dev.fit(data, use_labels=True)
    feats = [smp['features'].numpy() for smp in data._videos.values()]
    labels = [smp['gt_single'].numpy() for smp in data._videos.values()]
    want = O.fit_supervised(feats, labels, data.corpus.n_classes, data.max_k)
    sd_h, sd_d = host.model.state_dict(), dev.model.state_dict()
    for name in ('poisson_log_rates', 'gaussian_means', 'gaussian_cov', 'transition_logits', 'init_logits'):
        assert sd_d[name].is_cuda
        np.testing.assert_allclose(sd_d[name].cpu().numpy(), sd_h[name].numpy(), rtol=2e-6, atol=1e-7, err_msg=name)
    np.testing.assert_allclose(sd_d['gaussian_means'].cpu().numpy(), want['gaussian_means'], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(sd_d['poisson_log_rates'].cpu().numpy(), want['poisson_log_rates'], rtol=2e-6, atol=1e-7)


def test_out_of_range_label_is_an_error():
    from action_segmentation_amd.semimarkov_utils import semimarkov_sufficient_stats_device
    x = [torch.zeros(5, 8)]
    y = [torch.tensor([0, 1, 9, 1, 0])]
    with pytest.raises(ValueError, match="outside"):
        semimarkov_sufficient_stats_device(x, y, 'tied_diag', 4, 5)


def test_out_of_range_label_late_in_a_long_video_is_an_error():
    """The error word is raised from the second chunk of a video (frame 3000 of 4100); the bad frame is counted nowhere."""
    y = np.zeros(4100, dtype=np.int64)
    y[1500:] = 3
    y[3000] = -1
    with pytest.raises(ValueError, match="outside"):
        device_stats([np.zeros((4100, 4), dtype=np.float32)], [y], 4, 20)


def test_out_of_range_label_in_a_late_video_is_an_error():
    """... and from video 900 of 1000 (tests/fit_cases.py: many_items_labels), one of 1002 chunks."""
    labels = [y.copy() for y in F.many_items_labels()]
    labels[900][-1] = F.MANY_CLASSES
    feats = [np.zeros((len(y), 4), dtype=np.float32) for y in labels]
    with pytest.raises(ValueError, match="outside"):
        device_stats(feats, labels, F.MANY_CLASSES, F.MANY_MAX_K)
