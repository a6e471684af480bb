"""The premise of test_gpu_fit.py's chunk-carry cases, on the host: the run lists of tests/fit_cases.py make the start of
the run that is open at a chunk's first frame observable in the span counts.  A restatement of smm_span_stats_kernel's
chunked rule (fit_cases.chunked_span_stats) equals oracle.dense_ref.sufficient_stats with the true carry and differs from
it with either wrong one -- so a kernel whose backward scan returned a wrong start could not pass the GPU test."""
import numpy as np
import pytest

import fit_cases as F
from oracle import dense_ref as O


@pytest.fixture(scope='module')
def oracle_counts():
    feats, labels = F.carry_batch()
    # (the integer statistics do not depend on the features; one column keeps the oracle's one-hot product small)
    thin = [f[:, :1] for f in feats]
    batch = {mk: O.sufficient_stats(thin, labels, F.N_CLASSES, mk) for mk in F.MAX_KS}
    video = {(name, mk): O.sufficient_stats([thin[i]], [labels[i]], F.N_CLASSES, mk)
             for i, name in enumerate(F.CARRY_NAMES) for mk in F.CARRY_MAX_KS}
    return batch, video


def test_run_lists_are_what_the_cases_claim():
    _, labels = F.carry_batch()
    y = dict(zip(F.CARRY_NAMES, labels))
    assert len(y['straddle']) == 4396
    assert F.run_start_before(y['straddle'], 2048) == 2048 - 348          # second trip of the 256-label scan
    assert y['straddle'][4095] != y['straddle'][4096]                      # a change exactly at c_begin
    assert len(y['whole']) == 2 * F.CHUNK + 5 and len(set(y['whole'].tolist())) == 1
    assert F.run_start_before(y['whole'], 2048) == 0 and F.run_start_before(y['whole'], 4096) == 0
    assert F.run_start_before(y['tid0'], 2048) == 2047                     # first lane of the first trip
    assert F.run_start_before(y['trip_edge'], 2048) == 2048 - F.SCAN
    assert F.run_start_before(y['trip_edge'], 4096) == 4096 - F.SCAN - 1
    assert all(0 <= int(v.min()) and int(v.max()) < F.N_CLASSES for v in labels)


@pytest.mark.parametrize('max_k', F.MAX_KS)
def test_chunked_rule_with_the_true_carry_is_the_oracle(oracle_counts, max_k):
    _, labels = F.carry_batch()
    got = F.chunked_span_stats(labels, F.N_CLASSES, max_k, 'true')
    for key in F.INT_KEYS:
        np.testing.assert_array_equal(got[key], oracle_counts[0][max_k][key], err_msg=key)


@pytest.mark.parametrize('max_k', (None, 2))
@pytest.mark.parametrize('carry', F.WRONG_CARRIES)
def test_control_settings_do_not_see_the_carry(oracle_counts, carry, max_k):
    _, labels = F.carry_batch()
    assert F.same_counts(F.chunked_span_stats(labels, F.N_CLASSES, max_k, carry), oracle_counts[0][max_k])


@pytest.mark.parametrize('max_k', F.CARRY_MAX_KS)
@pytest.mark.parametrize('carry', F.WRONG_CARRIES)
def test_a_wrong_carry_changes_the_counts_of_the_batch(oracle_counts, carry, max_k):
    _, labels = F.carry_batch()
    got = F.chunked_span_stats(labels, F.N_CLASSES, max_k, carry)
    assert not F.same_counts(got, oracle_counts[0][max_k])
    np.testing.assert_array_equal(got['span_lengths'], oracle_counts[0][max_k]['span_lengths'])   # frames: no carry in them


@pytest.mark.parametrize('name', F.CARRY_NAMES)
def test_every_video_is_caught_by_some_wrong_carry(oracle_counts, name):
    _, labels = F.carry_batch()
    y = labels[F.CARRY_NAMES.index(name)]
    caught = [(carry, mk) for carry in F.WRONG_CARRIES for mk in F.CARRY_MAX_KS
              if not F.same_counts(F.chunked_span_stats([y], F.N_CLASSES, mk, carry), oracle_counts[1][(name, mk)])]
    assert caught, name


def test_many_items_layout():
    labels = F.many_items_labels()
    assert len(labels) == 1000
    for pos, t in F.MANY_LONG.items():
        assert len(labels[pos]) == t
    assert all(1 <= len(y) <= 30 for i, y in enumerate(labels) if i not in F.MANY_LONG)
    items = sum(4 * -(-len(y) // F.CHUNK) for y in labels)
    assert items == 4008 and 5 * 768 < items < 6 * 768             # 1002 chunks: five to six work items per workgroup
    seen = set(np.concatenate(labels).tolist())
    assert seen == set(range(F.MANY_CLASSES)) - {F.MANY_ABSENT}
