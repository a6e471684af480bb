"""The reference's own test of the DP boundary, run through this package's torch_struct stand-in on the GPU,
plus numeric checks of the dense kernel against the oracle."""
import numpy as np
import pytest
import torch

from oracle import dense_ref as O

pytestmark = pytest.mark.gpu
BIG_NEG = -1e9


def test_log_hsmm_known_answer_like_the_reference_test():
    """src/models/test_semimarkov.py:266-323 (test_log_hsmm) with
    `from action_segmentation_amd.struct import SemiMarkov, MaxSemiring` in place of torch_struct."""
    from action_segmentation_amd.struct import SemiMarkov, MaxSemiring
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    device = torch.device('cuda:0')
    sm_max = SemiMarkov(MaxSemiring)
    b, C, N, K, step_length = 10, 4, 100, 5, 4
    padded_length = N + step_length * 2
    lengths_unpadded = torch.full((b,), N).long()
    lengths_unpadded[0] = padded_length
    lengths = lengths_unpadded + 1
    num_steps = N // step_length
    trans_scores = torch.zeros(C, C, device=device)
    init_scores = torch.full((C,), BIG_NEG, device=device)
    init_scores[0] = 0
    emission_scores = torch.full((b, padded_length, C), BIG_NEG, device=device)
    for n in range(padded_length):
        emission_scores[:, n, (n // step_length) % C] = 1
    length_scores = torch.full((K, C), BIG_NEG, device=device)
    length_scores[step_length, :] = 0
    scores = SemiMarkovModule.log_hsmm(trans_scores, emission_scores, init_scores, length_scores, lengths_unpadded,
                                       add_eos=True)
    marginals = sm_max.marginals(scores, lengths=lengths)
    sequence, extra = sm_max.from_parts(marginals)
    for step in range(num_steps):
        assert torch.allclose(sequence[:, step_length * step], torch.full((1,), step % C).long())
    assert torch.allclose(sequence[torch.arange(0, b), lengths - 1], torch.full((1,), C).long())


def check_dense_kernel(edge, lengths, integer):
    from action_segmentation_amd.struct import SemiMarkovCRF
    _, _, k, c, _ = edge.shape
    dist = SemiMarkovCRF(edge.cuda(), lengths=lengths)
    v, segs = O.viterbi_backpointers(edge.double(), lengths)
    parts = dist.argmax
    assert parts.shape == edge.shape
    np.testing.assert_allclose(dist.max.cpu().numpy(), v.numpy(), rtol=1e-6)
    if integer:
        np.testing.assert_array_equal(parts.cpu().numpy(), O.parts_from_segments(segs, edge.shape).numpy())
    seq, (c2, k2) = dist.struct.from_parts(parts)
    assert (c2, k2) == (c, k)
    np.testing.assert_allclose((edge * parts.cpu()).flatten(1).sum(1).numpy(), v.numpy(), rtol=1e-5, atol=1e-4)
    z, _ = O.semimarkov_dp(edge.double(), lengths, O.LogSemiring)
    np.testing.assert_allclose(dist.partition.cpu().numpy(), z.numpy(), rtol=1e-6)
    gold = dist.struct.to_parts(seq, (c, k), lengths)
    np.testing.assert_allclose(dist.log_prob(gold.cuda()).cpu().numpy(), (v - z).numpy(), rtol=1e-4, atol=1e-4)


def random_edge(g, shape, integer):
    """Dense potentials; ``integer``: a lattice of small integers, where ties order the back-pointers."""
    return torch.randint(-4, 1, shape, generator=g).float() if integer else torch.randn(*shape, generator=g)


@pytest.mark.parametrize('seed', range(4))
def test_dense_kernel_matches_oracle(seed):
    g = torch.Generator().manual_seed(seed)
    b, n, k, c = 3, 30 + seed, 6 + seed, 5
    integer = seed % 2 == 0                                         # exact ties every other seed
    edge = random_edge(g, (b, n - 1, k, c, c), integer)
    check_dense_kernel(edge, torch.tensor([n, n - 3, n - 1]), integer)


# Shapes beyond one trip of the kernels' strided loops (csrc/smm_dense.hip launches min(1024, K C rounded up to 64) threads):
#   (2, 80, 70, 16)  1120 (k, to) pairs on 1024 threads: 96 threads make a second trip of the alpha loop; the backward kernel
#                    has 64 slices of 16 `from`; K - 1 = 69 is above n for the first 69 positions and below it after them
#                    (and above the whole second instance but for its last 11 positions)
#   (2, 12, 3, 130)  C above two waves: 390 pairs on 448 threads, beta on 130 of them; 3 backward slices, 58 idle threads
WIDE = [((2, 80, 70, 16), [80, 41]), ((2, 12, 3, 130), [12, 7])]
WIDE_IDS = ['k70_c16', 'k3_c130']


@pytest.mark.parametrize('seed', range(2))
@pytest.mark.parametrize('shape,lengths', WIDE, ids=WIDE_IDS)
def test_dense_kernel_matches_oracle_beyond_one_trip(shape, lengths, seed):
    b, n, k, c = shape
    integer = seed % 2 == 0
    edge = random_edge(torch.Generator().manual_seed(10 + seed), (b, n - 1, k, c, c), integer)
    check_dense_kernel(edge, torch.tensor(lengths), integer)


def check_dense_gradient(edge, lengths, w):
    """Autograd through the dense boundary (reference: loss.backward() through torch_struct's LogSemiring DP,
    semimarkov.py:286 / semimarkov_modules.py:652-657) against autograd through the oracle DP, fp64."""
    from action_segmentation_amd.struct import SemiMarkovCRF, SemiMarkov, LogSemiring
    b, _, k, c, _ = edge.shape
    z, want = O.marginals(edge.double(), lengths, O.LogSemiring)
    got = SemiMarkov(LogSemiring).marginals(edge.cuda(), lengths=lengths)
    assert got.shape == edge.shape and got.dtype == edge.dtype
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=1e-7)
    # every position but the last is covered by exactly one span: expected span mass per instance = 1 at n = 0
    np.testing.assert_allclose(got[:, 0].flatten(1).sum(1).cpu().numpy(), np.ones(b), rtol=1e-5)
    # weighted upstream gradient + chain rule through a parameter
    scale = torch.tensor(0.7, requires_grad=True)
    e_dev = edge.cuda().requires_grad_(True)
    dist = SemiMarkovCRF(e_dev * scale.cuda(), lengths=lengths)
    loss = (dist.partition * w.cuda()).sum()
    loss.backward()
    e_ref = edge.double().requires_grad_(True)
    s_ref = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    z_ref, _ = O.semimarkov_dp(e_ref * s_ref, lengths, O.LogSemiring)
    (z_ref * w.double()).sum().backward()
    np.testing.assert_allclose(e_dev.grad.cpu().numpy(), e_ref.grad.numpy(), rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(scale.grad.item(), s_ref.grad.item(), rtol=1e-4)
    # log_prob is differentiable too (reference log_likelihood: dist.log_prob(parts).mean())
    gold = dist.struct.to_parts(SemiMarkovCRF(edge.cuda(), lengths=lengths).struct.from_parts(
        SemiMarkovCRF(edge.cuda(), lengths=lengths).argmax)[0], (c, k), lengths)
    e2 = edge.cuda().requires_grad_(True)
    SemiMarkovCRF(e2, lengths=lengths).log_prob(gold.cuda()).sum().backward()
    np.testing.assert_allclose(e2.grad.cpu().numpy(), (gold.double() - want).numpy(), rtol=5e-5, atol=1e-6)


@pytest.mark.parametrize('seed', range(4))
def test_dense_partition_gradient_and_log_marginals(seed):
    g = torch.Generator().manual_seed(100 + seed)
    b, n, k, c = 3, 24 + 5 * seed, 4 + 3 * seed, 3 + 2 * seed
    edge = torch.randn(b, n - 1, k, c, c, generator=g)
    if seed == 3:
        edge[:, :, :, 1, :] = BIG_NEG                               # a forbidden label
    check_dense_gradient(edge, torch.tensor([n, n - 4, 2]), torch.tensor([0.5, -2.0, 3.0]))


@pytest.mark.parametrize('seed', range(2))
@pytest.mark.parametrize('shape,lengths', WIDE, ids=WIDE_IDS)
def test_dense_partition_gradient_beyond_one_trip(shape, lengths, seed):
    b, n, k, c = shape
    edge = random_edge(torch.Generator().manual_seed(110 + seed), (b, n - 1, k, c, c), seed % 2 == 0)
    check_dense_gradient(edge, torch.tensor(lengths), torch.tensor([0.5, -2.0]))


def test_dense_instance_of_length_one():
    """lengths = [n, 1]: no edge belongs to the second instance.  Its value is `plus` over beta[0] = one (log C under the Log
    semiring, 0 under Max), its span row holds position 0 only, and it has no posterior mass."""
    from action_segmentation_amd.struct import SemiMarkovCRF, SemiMarkov, LogSemiring, _dense_dp
    b, n, k, c = 2, 6, 4, 3
    edge = torch.randn(b, n - 1, k, c, c, generator=torch.Generator().manual_seed(5))
    lengths = torch.tensor([n, 1])
    dist = SemiMarkovCRF(edge.cuda(), lengths=lengths)
    v, segs = O.viterbi_backpointers(edge.double(), lengths)
    z, want = O.marginals(edge.double(), lengths, O.LogSemiring)
    assert segs[1] == [] and float(v[1]) == 0.0 and abs(float(z[1]) - np.log(c)) < 1e-15
    assert float(want[1].abs().sum()) == 0.0
    np.testing.assert_allclose(dist.max.cpu().numpy(), v.numpy(), rtol=1e-6)
    np.testing.assert_allclose(dist.partition.cpu().numpy(), z.numpy(), rtol=1e-6)
    assert float(dist.max[1]) == 0.0
    _, spans = _dense_dp(edge.cuda(), lengths, False, True)
    spans = spans.cpu()
    np.testing.assert_array_equal(spans[0].numpy(), O.spans_from_segments(segs, n)[0].numpy())
    assert int(spans[1, 0]) == 0                                    # torch.max order: the smallest final label
    assert spans[1, 1:].tolist() == [-1] * (n - 1)
    parts = dist.argmax
    assert float(parts[1].abs().sum()) == 0.0
    got = SemiMarkov(LogSemiring).marginals(edge.cuda(), lengths=lengths)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=1e-7)
    assert float(got[1].abs().sum()) == 0.0
    e = edge.cuda().requires_grad_(True)
    SemiMarkovCRF(e, lengths=lengths).partition.sum().backward()
    assert float(e.grad[1].abs().sum()) == 0.0


def test_dense_marginals_reference_shape():
    """Reference-size lattice (K = 20, C = 13 incl. EOS, N = 300): marginal mass is conserved at every position."""
    from action_segmentation_amd.struct import SemiMarkov, LogSemiring
    g = torch.Generator().manual_seed(7)
    b, n, k, c = 2, 300, 20, 13
    edge = torch.randn(b, n - 1, k, c, c, generator=g).cuda()
    lengths = torch.tensor([n, n - 37])
    m = SemiMarkov(LogSemiring).marginals(edge, lengths=lengths).double()
    # position p is covered by exactly one span [s, s + k'): sum over spans covering p == 1 (for p < L - 1)
    per_nk = m.sum(dim=(3, 4))                                      # b x (n-1) x k
    cover = torch.zeros(b, n - 1, dtype=torch.float64, device=m.device)
    for kk in range(1, k):
        for off in range(kk):
            cover[:, off:] += per_nk[:, :n - 1 - off, kk]
    for i, L in enumerate(lengths.tolist()):
        np.testing.assert_allclose(cover[i, :L - 1].cpu().numpy(), np.ones(L - 1), rtol=1e-4)
        assert float(m[i, L - 1:].abs().sum()) == 0.0
