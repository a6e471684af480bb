"""Forced alignment with optional entries on a bench corpus, timed as scripts/prof_align.py times (HIP events around the calls,
medians of 5; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times):
  (i)   every video's own Viterbi transcript with no flag set, through smm_align_opt_f64, beside smm_align_f64 on the same
        inputs -- the yardstick;
  (ii)  the same transcripts with an optional entry of a random class between every two entries and at both ends (the
        CrossTask shape "bg, step, bg, ..., bg": M -> 2 M + 1);
  (iii) for the videos whose transcript of (ii) has at most 32 entries, smm_viterbi_f64 on the expanded lattice of (ii) -- the
        only way to get this result before.
The summary line is printed and appended to profiles/align_opt_kernel_times.txt (or to the file given as the second argument).
usage: python scripts/prof_align_optional.py [cfg3|cfg2|cfg4|refdef] [out.txt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth
from action_segmentation_amd.semimarkov_utils import spans_to_transcripts

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg2'
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
t, B = pc.tables, pc.batch
elp, _ = ops.emission(B, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
vit = ops.viterbi(B, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, want_labels=False)   # (no class map: local ids)
torch.cuda.synchronize()
ops.check_decoded(B, vit)
tr = spans_to_transcripts(vit['spans'], B.lengths)
group = B.group if B.group is not None else np.zeros(B.b, np.int32)
kp = B.kp if B.kp is not None else np.full(B.b, min(B.k_rows, B.t_max), np.int32)
rng = np.random.default_rng(0)


def sub(keep, transcripts, flags):
    """The launch of the videos `keep`: batch, transcripts, flags, endpen rows, a workspace for either entry point."""
    batch = ops.Batch(B.lengths[keep], B.n_states, B.k_rows, c_max=B.c_max, frame_offset=B.frame_offset[keep], group=group[keep],
                      kp=kp[keep], t_max=B.t_max, total_frames=B.total_frames)
    tra, fl = [transcripts[i] for i in keep], [flags[i] for i in keep]
    ep = None if pc.endpen is None else pc.endpen[torch.as_tensor(keep, device=dev)].contiguous()
    off = np.concatenate([[0], np.cumsum([len(x) for x in tra])]).astype(np.int64)
    ws = torch.empty(ops.align_opt_workspace_bytes(batch, off), dtype=torch.uint8, device=dev)
    return batch, tra, fl, ep, ws


def align(s):
    return ops.align(s[0], elp, t['trans'], t['init'], t['len'], s[1], endpen=s[3], ws=s[4], want_labels=False)


def align_opt(s):
    return ops.align_optional(s[0], elp, t['trans'], t['init'], t['len'], s[1], s[2], endpen=s[3], ws=s[4], want_labels=False)


# (i) no flag set
ms1 = np.array([len(x) for x in tr])
s1 = sub(np.flatnonzero(ms1 <= ops.MAX_TRANSCRIPT), tr, [np.zeros(len(x), bool) for x in tr])
# (ii) an optional entry of a random class of the video between every two entries and at both ends
tr2, fl2 = [], []
for i, x in enumerate(tr):
    y = rng.integers(0, B.n_states[group[i]], size=2 * len(x) + 1)
    y[1::2] = x
    tr2.append(y)
    fl2.append(np.arange(len(y)) % 2 == 0)
ms2 = np.array([len(x) for x in tr2])
s2 = sub(np.flatnonzero(ms2 <= ops.MAX_TRANSCRIPT), tr2, fl2)
# (iii) the expanded lattice of (ii) for the videos with at most 32 entries: one parameter group per video
small = np.flatnonzero(ms2 <= 32)
lat = None
if small.size:
    n, cm, K = small.size, 32, B.k_rows
    th, ih, lh = t['trans'].cpu().numpy(), t['init'].cpu().numpy(), t['len'].cpu().numpy()
    eh = None if pc.endpen is None else pc.endpen.cpu().numpy()
    lengths = B.lengths[small]
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    e2 = torch.zeros((int(lengths.sum()), cm), dtype=torch.float64, device=dev)
    t2, i2 = np.full((n, cm, cm), -1e9), np.full((n, cm), -1e9)
    l2, p2 = np.zeros((n, K, cm)), np.full((n, cm), -1e9)
    for j, i in enumerate(small):
        g, ids, M = int(group[i]), tr2[i], len(tr2[i])
        o = int(B.frame_offset[i])
        e2[offs[j]:offs[j] + lengths[j], :M] = elp[o:o + int(lengths[j])][:, torch.as_tensor(ids, device=dev)]
        l2[j, :, :M] = lh[g][:, ids]
        for m in range(M):
            # even entries are optional: pred(m) = {m-1} behind a mandatory entry, {m-1, m-2} behind an optional one
            for q in ((m - 1,) if m % 2 == 0 else (m - 1, m - 2)):
                if q >= 0:
                    t2[j, m, q] = th[g, ids[m], ids[q]]
            if m <= 1:
                i2[j, m] = ih[g, ids[m]]
            if m >= M - 2:
                p2[j, m] = 0.0 if eh is None else eh[i, ids[m]]
    Bl = ops.Batch(lengths, ms2[small], K, c_max=cm, frame_offset=offs, group=np.arange(n, dtype=np.int32), kp=kp[small],
                   t_max=int(lengths.max()), total_frames=int(lengths.sum()))
    lat = (Bl, e2) + tuple(torch.from_numpy(x).to(dev) for x in (t2, i2, l2, p2))


def lattice():
    return ops.viterbi(lat[0], lat[1], lat[2], lat[3], lat[4], endpen=lat[5], want_labels=False)


o0, o1, o2 = align(s1), align_opt(s1), align_opt(s2)
torch.cuda.synchronize()
for s, o in ((s1, o0), (s1, o1), (s2, o2)):
    ops.check_decoded(s[0], o)
same = bool(torch.equal(o0['best'], o1['best']) and torch.equal(o0['spans'], o1['spans']))
pos = {int(v): j for j, v in enumerate(np.flatnonzero(ms2 <= ops.MAX_TRANSCRIPT))}
same_lat = None
if lat is not None:
    lv = lattice()
    torch.cuda.synchronize()
    same_lat = bool(torch.equal(lv['best'], o2['best'][torch.as_tensor([pos[int(i)] for i in small], device=dev)]))
times = [[], [], [], []]
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    e[0].record()
    align(s1)
    e[1].record()
    align_opt(s1)
    e[2].record()
    align_opt(s2)
    e[3].record()
    if lat is not None:
        lattice()
    e[4].record()
    torch.cuda.synchronize()
    for q in range(4):
        times[q].append(e[q].elapsed_time(e[q + 1]))
med = [float(np.median(x)) for x in times]
line = ('%s: %d videos, %d frames, longest %d; Viterbi transcripts: median %d, longest %d entries; (i) no flags, %d videos: '
        'align call %.3f ms, align_optional call %.3f ms, equal: %s; (ii) an optional entry between every two and at both ends '
        '(median %d entries), %d videos: align_optional call %.3f ms; (iii) viterbi on the expanded lattices of the %d videos of '
        '(ii) with <= 32 entries (%d frames) %.3f ms, equal: %s (medians of 5)'
        % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms1)), int(ms1.max()), len(s1[1]), med[0],
           med[1], same, int(np.median(ms2)), len(s2[1]), med[2], small.size, int(B.lengths[small].sum()) if small.size else 0,
           med[3], same_lat))
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_opt_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
