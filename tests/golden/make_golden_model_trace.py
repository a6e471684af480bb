"""Golden trace of the model layer's transcript family: what ``SemiMarkovModel`` hands to the packed entry points of its module
for a transcript-supervised call, and what it returns.

    python tests/golden/make_golden_model_trace.py            ->  tests/golden/model_transcript_trace.json   (committed)
    python tests/golden/make_golden_model_trace.py --show ID  ->  the full trace of one case on stdout (for a diff)

No GPU and no library: the model's module and its ``prepare`` are replaced by recording fakes.  ``prepare`` hands out a corpus
of three named videos; the module's entry points return values computed from the CONTENT of what they are given: the score of
a class sequence on a video is a hash of (video, sequence), so no two different sequences tie; a graph's value is taken over
the class sequences of its start -> end paths; a sample is a hash of (seed, video, j).  The frame labels of a class sequence
spread its entries evenly over the video.

The committed table was made from ``semimarkov.py`` exactly as it stood in front of the refactor that gave the per-video
look-up of the supervision, the slicing of the labels and the chunking of the candidates one statement each;
tests/test_model_host.py holds every later model to it.  Every case keeps the calls and the result, except
``align_candidates``: its result and the number of its launches.  The tries it hands over are not kept: a candidate that comes
again behind a split of its video's list is in the later trie or is not, and the result -- the best over the DISTINCT class
sequences, a duplicate answering to its lowest index -- cannot tell.
"""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "model_transcript_trace.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_CLASSES = 12
NAMES = ['v_b', 'v_a', 'v_c']                               # (the corpus's order, not the alphabet's)
LENGTHS = [8, 5, 7]
OFFSETS = [0, 9, 14]                                        # frame 8 belongs to no video


def _unit(*key):
    """A hash of ``key`` in [0, 1)."""
    return int(hashlib.sha1(repr(key).encode()).hexdigest()[:12], 16) / float(1 << 48)


def _score(video, seq):
    return -10.0 * _unit('score', video, tuple(int(c) for c in seq)) - 1.0


def _ints(a):
    return [int(v) for v in np.asarray(a.cpu() if torch.is_tensor(a) else a).reshape(-1)]


def _paths(graph):
    """Every start -> end path of a graph, as node lists, in the order of the end node and then of the predecessors."""
    out = []

    def back(m, tail):
        tail = [m] + tail
        if graph.start[m]:
            out.append(tail)
        for j in np.flatnonzero(graph.pred[m]):
            back(int(j), tail)
    for m in np.flatnonzero(graph.end):
        back(int(m), [])
    return out


def _spread(seq, t):
    return [int(seq[(f * len(seq)) // t]) for f in range(t)] if len(seq) <= t else [-1] * t


class FakeModule:
    """The packed entry points ``SemiMarkovModel`` calls, computed from the content of their arguments; every call is kept."""
    n_classes = N_CLASSES

    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def _note(self, name, **kw):
        self.calls.append(dict(kw, entry=name))

    @staticmethod
    def _graph(g):
        return {k: np.asarray(getattr(g, k)).astype(np.int64).tolist() for k in ('ids', 'start', 'end', 'end_candidate')} | {
            'pred': [np.flatnonzero(row).tolist() for row in g.pred]}

    @staticmethod
    def _labels(pc, rows, lead=()):
        lab = np.full(lead + (OFFSETS[-1] + LENGTHS[-1],), -1, np.int64)
        for (off, t), row in zip(zip(pc.frame_offset, pc.lengths), rows):
            lab[..., off:off + t] = row
        return torch.from_numpy(lab)

    def _kept(self, v, seq, flags):
        """The best subset of the optional entries: the highest-scoring class sequence among all of them."""
        seq, flags = _ints(seq), [False] * len(_ints(seq)) if flags is None else [bool(f) for f in _ints(flags)]
        subsets = [[]]
        for c, f in zip(seq, flags):
            subsets = [s + [c] for s in subsets] + ([s for s in subsets] if f else [])
        return max((s for s in subsets if s), key=lambda s: _score(v, s))

    def align_packed(self, pc, transcripts, optional=None):
        self._note('align_packed', transcripts=[_ints(t) for t in transcripts],
                   optional=None if optional is None else [_ints(f) for f in optional])
        best = [self._kept(v, t, None if optional is None else optional[v]) for v, t in enumerate(transcripts)]
        return (self._labels(pc, [_spread(s, t) for s, t in zip(best, pc.lengths)]),
                torch.tensor([_score(v, s) for v, s in enumerate(best)], dtype=torch.float64))

    def align_graph_packed(self, pc, graphs):
        self._note('align_graph_packed', graphs=[self._graph(g) for g in graphs])
        rows, scores, used = [], [], []
        for v, g in enumerate(graphs):
            paths = [p for p in _paths(g) if len(p) <= pc.lengths[v]]
            u = np.zeros(len(g), np.int32)
            if paths:
                best = max(paths, key=lambda p: _score(v, g.ids[p]))
                u[best] = 1
                rows.append(_spread(g.ids[best], pc.lengths[v]))
                scores.append(_score(v, g.ids[best]))
            else:
                rows.append([-1] * pc.lengths[v])
                scores.append(float('-inf'))
            used.append(torch.from_numpy(u))
        return self._labels(pc, rows), torch.tensor(scores, dtype=torch.float64), used

    def _graph_logz(self, pc, v, g):
        s = [_score(v, g.ids[p]) for p in _paths(g) if len(p) <= pc.lengths[v]]
        return float(np.logaddexp.reduce(s)) if s else float('-inf')

    def transcript_graph_scores_packed(self, pc, graphs, conditional=False, ambiguous='raise'):
        self._note('transcript_graph_scores_packed', graphs=[self._graph(g) for g in graphs], conditional=conditional,
                   ambiguous=ambiguous)
        return torch.tensor([self._graph_logz(pc, v, g) - (_unit('logz', v) if conditional else 0.0) for v, g in enumerate(graphs)],
                            dtype=torch.float64)

    def transcript_node_posteriors_packed(self, pc, graphs):
        self._note('transcript_node_posteriors_packed', graphs=[self._graph(g) for g in graphs])
        p_used, p_end = [], []
        for v, g in enumerate(graphs):
            z, pu, pe = self._graph_logz(pc, v, g), np.zeros(len(g)), np.zeros(len(g))
            for p in _paths(g):
                if len(p) <= pc.lengths[v]:
                    w = np.exp(_score(v, g.ids[p]) - z)
                    pu[p] += w
                    pe[p[-1]] += w
            p_used.append(pu)
            p_end.append(pe)
        return p_used, p_end

    def sample_alignments_packed(self, pc, graphs, n_samples, seed=0):
        self._note('sample_alignments_packed', graphs=[self._graph(g) for g in graphs], n_samples=n_samples, seed=seed)
        rows, used, logp = [], [], np.zeros((n_samples, len(graphs)))
        for v, g in enumerate(graphs):
            paths = [p for p in _paths(g) if len(p) <= pc.lengths[v]]
            u, lab = np.zeros((n_samples, len(g)), np.int32), np.full((n_samples, pc.lengths[v]), -1, np.int64)
            for j in range(n_samples if paths else 0):
                p = paths[int(_unit('draw', seed, v, j) * len(paths))]
                u[j, p] = 1
                lab[j] = _spread(g.ids[p], pc.lengths[v])
                logp[j, v] = _score(v, g.ids[p]) - self._graph_logz(pc, v, g)
            rows.append(lab)
            used.append(torch.from_numpy(u))
        return self._labels(pc, rows, (n_samples,)), torch.from_numpy(logp), used

    def transcript_scores_packed(self, pc, transcripts, conditional=False, optional=None, ambiguous='raise'):
        self._note('transcript_scores_packed', transcripts=[_ints(t) for t in transcripts], conditional=conditional,
                   optional=None if optional is None else [_ints(f) for f in optional], ambiguous=ambiguous)
        return torch.tensor([_score(v, _ints(t) + ([] if optional is None else [-1] + _ints(optional[v])))
                             - (_unit('logz', v) if conditional else 0.0) for v, t in enumerate(transcripts)], dtype=torch.float64)

    def transcript_entry_posteriors_packed(self, pc, transcripts, optional, ambiguous='raise'):
        self._note('transcript_entry_posteriors_packed', transcripts=[_ints(t) for t in transcripts],
                   optional=[_ints(f) for f in optional], ambiguous=ambiguous)
        return [np.array([_unit('entry', v, _ints(t), m) if f else 1.0 for m, f in enumerate(_ints(optional[v]))])
                for v, t in enumerate(transcripts)]


def fake_model():
    """A ``SemiMarkovModel`` over the fakes -> (model, module)."""
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    module = FakeModule()
    model = SemiMarkovModel(types.SimpleNamespace(cuda=False), N_CLASSES, 3, module)
    pc = types.SimpleNamespace(video_names=list(NAMES), lengths=list(LENGTHS), frame_offset=list(OFFSETS), n_videos=len(NAMES))
    model.prepare = lambda data, shard=None: pc
    return model, module


# -------------------------------------------------------------------------------------------------- the cases
TRANSCRIPTS = {'v_a': [3, 1, 3], 'v_b': torch.tensor([0, 1, 2, 1]), 'v_c': np.array([4, 5]), 'not in the corpus': [7]}
FLAGS = {'v_a': [0, 1, 0], 'v_b': torch.tensor([1, 0, 1, 0]), 'v_c': [False, False], 'not in the corpus': [1]}
CANDIDATES = {'v_a': [[3, 1], [3, 1, 3], [3, 1], [2]], 'v_b': [torch.tensor([0, 1, 2]), [0, 1], [1]], 'v_c': [[4, 5], [4, 5]]}


def _split_candidates():
    """Candidate lists whose tries exceed ``ops.MAX_TRANSCRIPT`` nodes.  ``v_b``: three tries at least -- a duplicate in front
    of the first split, one of the first candidate behind it and one of a middle candidate at the very end --, ``v_a``: two
    tries, ``v_c``: one.  The long candidates cover more entries than a video has frames: the short ones win."""
    from action_segmentation_amd import ops
    long = lambda c, n=ops.MAX_TRANSCRIPT // 2 - 20: [c] * n              # n trie nodes, shared with nothing
    return {'v_b': [[0, 1, 2], long(3), [0, 1, 2], [0, 2], long(4), long(5), [0, 1, 2], [1, 2, 1], long(6), [6, 6], long(8), long(4), [0, 2]],
            'v_a': [long(1), [1, 2], long(2), long(3), [1, 2], [2, 1]],
            'v_c': [[4, 5], long(7), [4, 5], [5]]}


def cases():
    """[(case id, fn(model) -> result, whether the calls are kept whole)]"""
    by_video = dict(optional_by_video=FLAGS)
    by_class = dict(optional_classes=[1, 5, 1])
    return [
        ('align', lambda m: m.align(None, TRANSCRIPTS), True),
        ('align|optional_by_video', lambda m: m.align(None, TRANSCRIPTS, **by_video), True),
        ('align|optional_classes', lambda m: m.align(None, TRANSCRIPTS, **by_class), True),
        ('align_candidates', lambda m: m.align_candidates(None, CANDIDATES), False),
        ('align_candidates|split', lambda m: m.align_candidates(None, _split_candidates()), False),
        ('candidate_log_likelihood', lambda m: m.candidate_log_likelihood(None, CANDIDATES), True),
        ('candidate_log_likelihood|conditional|split', lambda m: m.candidate_log_likelihood(None, _split_candidates(), True), True),
        ('candidate_posteriors', lambda m: m.candidate_posteriors(None, CANDIDATES), True),
        ('candidate_posteriors|split', lambda m: m.candidate_posteriors(None, _split_candidates()), True),
        ('sample_alignments', lambda m: m.sample_alignments(None, TRANSCRIPTS, 3, seed=5), True),
        ('sample_alignments|optional_by_video', lambda m: m.sample_alignments(None, TRANSCRIPTS, 2, **by_video), True),
        ('sample_alignments|optional_classes', lambda m: m.sample_alignments(None, TRANSCRIPTS, 2, seed=1, **by_class), True),
        ('sample_candidates', lambda m: m.sample_candidates(None, CANDIDATES, 4, seed=9), True),
        ('transcript_log_likelihood', lambda m: m.transcript_log_likelihood(None, TRANSCRIPTS), True),
        ('transcript_log_likelihood|conditional|optional_by_video',
         lambda m: m.transcript_log_likelihood(None, TRANSCRIPTS, True, **by_video), True),
        ('transcript_log_likelihood|optional_classes|allow',
         lambda m: m.transcript_log_likelihood(None, TRANSCRIPTS, ambiguous='allow', **by_class), True),
        ('transcript_entry_posteriors|optional_by_video', lambda m: m.transcript_entry_posteriors(None, TRANSCRIPTS, **by_video), True),
        ('transcript_entry_posteriors|optional_classes', lambda m: m.transcript_entry_posteriors(None, TRANSCRIPTS, **by_class), True),
    ]


def plain(v):
    """A result as JSON: arrays and tensors as lists, floats rounded to 9 decimals (the last bit of an exp differs between CPUs)."""
    if isinstance(v, dict):
        return {str(k): plain(e) for k, e in v.items()}
    if isinstance(v, (tuple, list)):
        return [plain(e) for e in v]
    if torch.is_tensor(v) or isinstance(v, np.ndarray):
        return plain(np.asarray(v.cpu() if torch.is_tensor(v) else v).tolist())
    if isinstance(v, (float, np.floating)):
        return repr(float(v)) if not np.isfinite(v) else round(float(v), 9)
    if isinstance(v, np.integer):
        return int(v)
    return v


def trace(fn, whole):
    model, module = fake_model()
    result = plain(fn(model))
    calls = plain(module.calls)
    digest = hashlib.sha1(json.dumps(calls, sort_keys=True, separators=(',', ':')).encode()).hexdigest()[:12]
    return {'entries': [c['entry'] for c in calls], 'calls': digest if whole else None, 'result': result}, calls


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--show':
        _, fn, whole = next(c for c in cases() if c[0] == sys.argv[2])
        row, calls = trace(fn, whole)
        print(json.dumps({'calls': calls, 'result': row['result']}, indent=1, sort_keys=True))
        return
    table = [dict(trace(fn, whole)[0], case=cid) for cid, fn, whole in cases()]
    with open(OUT, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(r, sort_keys=True, separators=(',', ':')) for r in table) + '\n]\n')
    print('%d cases -> %s' % (len(table), OUT))


if __name__ == '__main__':
    main()
