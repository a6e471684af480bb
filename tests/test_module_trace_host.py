"""The module layer against tests/golden/module_launch_trace.json (no GPU): every entry point of ``SemiMarkovModule`` calls the
launchers of ``ops`` in the recorded order with the recorded arguments -- the ``Batch`` and its flags, which earlier output each
tensor is, which workspace, every keyword -- and returns what it returned.  The padded and the packed twin of an operation differ
in ways no review sees (``no_time_split``, ``with_backward``, who checks the lengths); the table pins them.  A case that differs:
``python tests/golden/make_golden_module_trace.py --show CASE`` on both sides prints the full traces."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from action_segmentation_amd import ops, semimarkov_modules as smm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_module_trace", os.path.join(GOLDEN, "make_golden_module_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_points_launch_as_the_golden_trace():
    gen = _generator()
    with open(os.path.join(GOLDEN, "module_launch_trace.json")) as f:
        table = json.load(f)
    cases = gen.cases(smm)
    assert [r["case"] for r in table] == [cid for cid, _ in cases]          # the table is the generator's grid
    assert len(table) >= 500
    wrong = []
    for want, (cid, thunk) in zip(table, cases):
        got = gen.row(cid, gen.trace(smm, thunk))
        if got != want:
            wrong.append((want, got))
    assert not wrong, "%d cases differ, the first:\n%s\n%s" % (len(wrong), wrong[0][0], wrong[0][1])
    assert smm.ops is ops                                                    # (the stand-in is gone)


def test_golden_trace_covers_every_launcher_the_module_calls():
    with open(os.path.join(GOLDEN, "module_launch_trace.json")) as f:
        seen = {c.split(":")[0] for r in json.load(f) for c in r["calls"]}
    assert seen == {"emission", "emission_bwd", "decode", "logz", "logz_bwd", "sample", "entropy", "entropy_bwd", "kl", "kl_bwd",
                    "kbest", "mbr", "align", "check_decoded", "_err_copy", "align_optional", "align_graph", "align_logz",
                    "align_logz_ex", "align_logz_bwd", "align_opt_logz", "align_opt_logz_bwd", "align_graph_logz",
                    "align_graph_logz_bwd", "align_graph_sample"}


@pytest.mark.parametrize("name", ["kl_packed", "cross_entropy_packed"])
def test_kl_packed_leaves_the_corpus_prepared_for_self(name):
    gen = _generator()
    m, o, pack = gen.packed_setup(smm, True)
    pc = pack()
    m.prepare_packed(pc)
    before = (pc.batch, pc.tables, pc.endpen)
    assert before[2] is not None
    gen.trace(smm, lambda: getattr(m, name)(o, pc))
    assert pc.batch is before[0] and pc.tables is before[1] and pc.endpen is before[2]


SPAN = "one instance must span the padded length (padding_colate)"
NO_EOS = ("add_eos=False needs at least two frames per video (a one-frame video has no edge at all in the reference's lattice)")


def _refusals():
    """(id, exception type, exact text, fn(gen, m, other, i))"""
    short = lambda i: torch.tensor([5, 3, 2])            # no video spans Tmax = 6
    one = lambda i: torch.tensor([6, 1, 2])              # a one-frame video
    vc = lambda m, i: m._check_valid_classes(i.vcpi)
    rows = [
        ("span/_decode", AssertionError, SPAN, lambda g, m, o, i: m._decode(i.x, short(i), vc(m, i), None, None)),
        ("span/_posterior_launch", AssertionError, SPAN, lambda g, m, o, i: m.sample(i.x, short(i), i.vcpi)),
        ("span/viterbi_kbest", AssertionError, SPAN, lambda g, m, o, i: m.viterbi_kbest(i.x, short(i), i.vcpi, 2)),
        ("span/align", AssertionError, SPAN, lambda g, m, o, i: m.align(i.x, short(i), i.vcpi, i.transcripts)),
        ("span/log_partition", AssertionError, "", lambda g, m, o, i: m.log_partition(i.x, short(i), vc(m, i))),
        ("no_eos/_decode", ValueError, NO_EOS, lambda g, m, o, i: m._decode(i.x, one(i), vc(m, i), None, None, no_eos=True)),
        ("no_eos/_posterior_launch", ValueError, NO_EOS, lambda g, m, o, i: m.frame_posteriors(i.x, one(i), i.vcpi, False)),
        ("no_eos/viterbi_kbest", ValueError, NO_EOS, lambda g, m, o, i: m.viterbi_kbest(i.x, one(i), i.vcpi, 2, False)),
        ("no_eos/log_partition", ValueError, NO_EOS, lambda g, m, o, i: m.log_partition(i.x, one(i), vc(m, i), no_eos=True)),
        ("no_eos/align", ValueError, "align: add_eos=False is not supported",
         lambda g, m, o, i: m.align(i.x, i.lengths, i.vcpi, i.transcripts, False)),
        ("no_eos/align_packed", ValueError, "align_packed: add_eos=False is not supported",
         lambda g, m, o, i: m.align_packed(_no_eos_corpus(i), [[0]] * 3)),
        ("lattice/max_k", ValueError, "kl_divergence: the two posteriors must share the lattice: (n_classes, n_dims, max_k) "
         "(4, 3, 4) against (4, 3, 3)", lambda g, m, o, i: m.kl_divergence(g.padded_module(smm, True, 2, max_k=3), i.x, i.lengths, i.vcpi)),
        ("lattice/max_k/differentiable", ValueError, "cross_entropy: the two posteriors must share the lattice: (n_classes, n_dims, "
         "max_k) (4, 3, 4) against (4, 3, 3)",
         lambda g, m, o, i: m.cross_entropy(g.padded_module(smm, True, 2, max_k=3), i.x, i.lengths, i.vcpi, differentiable=True)),
        ("lattice/packed", ValueError, "kl_packed: the two posteriors must share the lattice: (n_classes, n_dims, max_k) "
         "(4, 3, 4) against (4, 3, 3)", lambda g, m, o, i: m.kl_packed(g.padded_module(smm, True, 2, max_k=3), None)),
        ("lattice/not a module", TypeError, "kl_divergence: other must be a SemiMarkovModule",
         lambda g, m, o, i: m.kl_divergence(object(), i.x, i.lengths, i.vcpi)),
        ("lattice/not a module/packed", TypeError, "cross_entropy_packed: other must be a SemiMarkovModule",
         lambda g, m, o, i: m.cross_entropy_packed(None, None)),
    ]
    batch = lambda lengths, **kw: ops.Batch(lengths, [3], 4, c_max=3, t_max=6, total_frames=18, d=3, **kw)
    differ = "kl_divergence: the two posteriors' batches differ (states, span limit or lengths)"
    for tag, other in (("lengths", batch([6, 3, 3])), ("no_eos", batch([6, 3, 2], no_eos=True)),
                       ("kp", batch([6, 3, 2], kp=[4, 4, 4])), ("group", batch([6, 3, 2], group=[0, 0, 0])),
                       ("k_rows", ops.Batch([6, 3, 2], [3], 5, c_max=3, t_max=6, total_frames=18, d=3)),
                       ("frame_offset", batch([6, 3, 2], frame_offset=[0, 6, 9]))):
        rows.append(("batch/" + tag, ValueError, differ,
                     lambda g, m, o, i, other=other: m._check_same_batch(batch([6, 3, 2]), other, "kl_divergence")))
    return rows + _transcript_refusals()


AMBIGUOUS = "%s: ambiguous must be 'raise' or 'allow'"
SUBSETS = ("%s: two subsets of the optional entries of video %r give the same class sequence, so its segmentations would be "
           "counted once per subset; pass ambiguous='allow' for that sum over alignments")
PATHS = ("%s: two start -> end paths of the graph of video %r spell the same class sequence, so its segmentations would be "
         "counted once per path; pass ambiguous='allow' for that sum over alignments")


def _transcript_refusals():
    """The host-side refusals of the fourteen entry points of the transcript family: five padded, nine packed."""
    G = ops.TranscriptGraph
    no_eos = "%s: add_eos=False is not supported"
    twice = lambda c: G([c, c], [[], []], [1, 1], [1, 1])         # two one-node paths that spell the same class
    rows = []
    add = lambda cid, text, fn, exc=ValueError: rows.append((cid, exc, text, fn))

    # ---- padded (videos are named by their index); i: three videos, valid classes 0, 1, 3
    tr = lambda i: (i.x, i.lengths, i.vcpi, i.transcripts)
    gr = lambda g, i: (i.x, i.lengths, i.vcpi, i.graphs(ops))
    add("no_eos/align_graph", no_eos % "align_graph", lambda g, m, o, i: m.align_graph(*gr(g, i), False))
    add("no_eos/transcript_log_partition", no_eos % "transcript_log_partition",
        lambda g, m, o, i: m.transcript_log_partition(*tr(i), False))
    add("no_eos/transcript_graph_log_partition", no_eos % "transcript_graph_log_partition",
        lambda g, m, o, i: m.transcript_graph_log_partition(*gr(g, i), False))
    add("no_eos/sample_alignments", no_eos % "sample_alignments", lambda g, m, o, i: m.sample_alignments(*gr(g, i), 2, 0, False))
    add("count/align", "align: 2 transcripts for 3 videos", lambda g, m, o, i: m.align(i.x, i.lengths, i.vcpi, i.transcripts[:2]))
    add("count/align_graph", "align_graph: 2 graphs for 3 videos",
        lambda g, m, o, i: m.align_graph(i.x, i.lengths, i.vcpi, i.graphs(ops)[:2]))
    add("count/transcript_log_partition", "transcript_log_partition: 2 transcripts for 3 videos",
        lambda g, m, o, i: m.transcript_log_partition(i.x, i.lengths, i.vcpi, i.transcripts[:2]))
    add("count/transcript_graph_log_partition", "transcript_graph_log_partition: 2 graphs for 3 videos",
        lambda g, m, o, i: m.transcript_graph_log_partition(i.x, i.lengths, i.vcpi, i.graphs(ops)[:2]))
    add("count/sample_alignments", "sample_alignments: 2 graphs for 3 videos",
        lambda g, m, o, i: m.sample_alignments(i.x, i.lengths, i.vcpi, i.graphs(ops)[:2]))
    add("flags/count/transcript_log_partition", "transcript_log_partition: 2 sequences of optional flags for 3 videos",
        lambda g, m, o, i: m.transcript_log_partition(*tr(i), optional=i.optional[:2]))
    add("flags/length/transcript_log_partition", "transcript_log_partition: 3 optional flags for the 2 transcript entries of video 1",
        lambda g, m, o, i: m.transcript_log_partition(*tr(i), optional=[[0, 1, 0], [0, 0, 0], [0, 0]]))
    add("ambiguous/word/transcript_log_partition", AMBIGUOUS % "transcript_log_partition",
        lambda g, m, o, i: m.transcript_log_partition(*tr(i), optional=i.optional, ambiguous="sum"))
    add("ambiguous/word/transcript_graph_log_partition", AMBIGUOUS % "transcript_graph_log_partition",
        lambda g, m, o, i: m.transcript_graph_log_partition(*gr(g, i), ambiguous="sum"))
    add("ambiguous/video/transcript_log_partition", SUBSETS % ("transcript_log_partition", 2),
        lambda g, m, o, i: m.transcript_log_partition(i.x, i.lengths, i.vcpi, [[0, 1, 3], [1, 3], [0, 0]],
                                                      optional=[[0, 1, 0], [0, 0], [1, 1]]))
    add("ambiguous/video/transcript_graph_log_partition", PATHS % ("transcript_graph_log_partition", 1),
        lambda g, m, o, i: m.transcript_graph_log_partition(i.x, i.lengths, i.vcpi, [G.chain([0]), twice(1), G.chain([3])]))
    add("graph/type/transcript_graph_log_partition", "transcript_graph_log_partition: an ops.TranscriptGraph expected for video 2",
        lambda g, m, o, i: m.transcript_graph_log_partition(i.x, i.lengths, i.vcpi, [G.chain([0]), G.chain([1]), [3]]))
    add("n_samples/sample_alignments", "sample_alignments: n_samples must be positive, got 0",
        lambda g, m, o, i: m.sample_alignments(*gr(g, i), 0))

    # ---- packed: four videos of two tasks, named; a corpus staged for add_eos=False has no video
    def on_corpus(call):
        def fn(g, m, o, i):
            pm, _, pack = g.packed_setup(smm, False)
            pc = pm.prepare_packed(pack())
            assert list(pc.video_names) == ["task00_v000", "task00_v001", "task01_v000", "task01_v001"]
            return call(pm, pc, g._transcripts(pm, pc), g._packed_graphs(pm, pc))
        return fn
    flags = [[0, 1, 0]] * 4
    with_transcripts = {
        "align_packed": lambda pm, pc, t, opt=None, **kw: pm.align_packed(pc, t, optional=opt, **kw),
        "transcript_log_partition_packed": lambda pm, pc, t, opt=None, **kw: pm.transcript_log_partition_packed(pc, t, optional=opt, **kw),
        "transcript_scores_packed": lambda pm, pc, t, opt=None, **kw: pm.transcript_scores_packed(pc, t, optional=opt, **kw),
        "transcript_entry_posteriors_packed": lambda pm, pc, t, opt=flags, **kw: pm.transcript_entry_posteriors_packed(pc, t, opt, **kw),
    }
    with_graphs = {
        "align_graph_packed": lambda pm, pc, gs, **kw: pm.align_graph_packed(pc, gs, **kw),
        "transcript_graph_log_partition_packed": lambda pm, pc, gs, **kw: pm.transcript_graph_log_partition_packed(pc, gs, **kw),
        "transcript_graph_scores_packed": lambda pm, pc, gs, **kw: pm.transcript_graph_scores_packed(pc, gs, **kw),
        "transcript_node_posteriors_packed": lambda pm, pc, gs, **kw: pm.transcript_node_posteriors_packed(pc, gs, **kw),
        "sample_alignments_packed": lambda pm, pc, gs, **kw: pm.sample_alignments_packed(pc, gs, 2, **kw),
    }
    for name, call in with_transcripts.items():
        if name != "align_packed":                                   # (in the table since the entry point came)
            add("no_eos/" + name, no_eos % name, lambda g, m, o, i, call=call: call(m, _no_eos_corpus(i), [], []))
        add("count/" + name, "align: 3 transcripts for 4 videos", on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, t[:3], flags[:3])))
        if name == "align_packed":                                   # (hands its flags to the launcher as they came)
            continue
        add("flags/count/" + name, "%s: 3 sequences of optional flags for 4 videos" % name,
            on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, t, flags[:3])))
        add("flags/length/" + name, "%s: 2 optional flags for the 3 transcript entries of video 'task00_v001'" % name,
            on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, t, [[0, 1, 0], [0, 1], [0, 1, 0], [0, 1, 0]])))
        add("ambiguous/word/" + name, AMBIGUOUS % name,
            on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, t, flags, ambiguous="sum")))
        add("ambiguous/video/" + name, SUBSETS % (name, "task01_v000"),
            on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, t[:2] + [[5, 5]] + t[3:], flags[:2] + [[1, 1]] + flags[3:])))
    add("flags/none/transcript_entry_posteriors_packed",
        "transcript_entry_posteriors_packed: one sequence of optional flags per video expected",
        on_corpus(lambda pm, pc, t, gs: pm.transcript_entry_posteriors_packed(pc, t, None)))
    for name, call in with_graphs.items():
        add("no_eos/" + name, no_eos % name, lambda g, m, o, i, call=call: call(m, _no_eos_corpus(i), []))
        add("count/" + name, "%s: 3 graphs for 4 videos" % ("align_graph" if name == "align_graph_packed" else name),
            on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, gs[:3])))
        if name in ("transcript_graph_log_partition_packed", "transcript_graph_scores_packed"):
            add("ambiguous/word/" + name, AMBIGUOUS % name, on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, gs, ambiguous="sum")))
            add("ambiguous/video/" + name, PATHS % (name, "task01_v001"),
                on_corpus(lambda pm, pc, t, gs, call=call: call(pm, pc, gs[:3] + [twice(5)])))
    add("n_samples/sample_alignments_packed", "sample_alignments_packed: n_samples must be positive, got 0",
        on_corpus(lambda pm, pc, t, gs: pm.sample_alignments_packed(pc, gs, 0)))
    return rows


def _no_eos_corpus(i):
    from action_segmentation_amd.batching import PackedCorpus
    pc = PackedCorpus()
    pc.x = i.x.view(-1, i.x.size(2))
    pc.batch = ops.Batch([6, 3, 2], [4], 4, no_eos=True)
    return pc


@pytest.mark.parametrize("cid,exc,text,fn", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_of_the_module_layer(cid, exc, text, fn):
    gen = _generator()
    m, o = gen.padded_module(smm, True, 1), gen.padded_module(smm, True, 2)
    i = gen.padded_inputs(True, False, False)
    with pytest.raises(exc) as e:
        gen.trace(smm, lambda: fn(gen, m, o, i))
    assert type(e.value) is exc and str(e.value) == text


def test_same_batch_accepts_equal_batches():
    mk = lambda: ops.Batch(np.array([6, 3, 2]), [3], 4, c_max=3, t_max=6, total_frames=18, d=3, kp=[4, 4, 4], group=[0, 0, 0])
    smm.SemiMarkovModule._check_same_batch(mk(), mk(), "kl_divergence")
