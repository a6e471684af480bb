"""Forced alignment on a bench corpus: every video is aligned to the transcript of its own Viterbi decode (smm_align_f64), beside
the Viterbi decode of the same corpus (smm_viterbi_f64) and -- for the videos whose transcript has at most 32 entries, the only
ones it can take -- smm_viterbi_f64 on the expanded lattice (states = transcript positions), which is how an alignment had to be
computed before smm_align_f64 existed.  HIP events here; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times
(smm_align_kernel beside smm_viterbi_kernel).  The summary line is printed and appended to profiles/align_kernel_times.txt (or
to the file given as the second argument).
usage: python scripts/prof_align.py [cfg3|cfg2|cfg4|refdef] [out.txt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth
from action_segmentation_amd.semimarkov_utils import spans_to_transcripts

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg3'
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
t, B = pc.tables, pc.batch
elp, _ = ops.emission(B, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)


def viterbi(batch, e, trans, init, lens, endpen):
    return ops.viterbi(batch, e, trans, init, lens, endpen=endpen, want_labels=False)


vit = viterbi(B, elp, t['trans'], t['init'], t['len'], pc.endpen)          # (no class map: the spans hold local ids)
torch.cuda.synchronize()
ops.check_decoded(B, vit)
tr = spans_to_transcripts(vit['spans'], B.lengths)
ms_len = np.array([len(x) for x in tr])
group = B.group if B.group is not None else np.zeros(B.b, np.int32)
kp = B.kp if B.kp is not None else np.full(B.b, min(B.k_rows, B.t_max), np.int32)


def sub_batch(keep):
    return ops.Batch(B.lengths[keep], B.n_states, B.k_rows, c_max=B.c_max, frame_offset=B.frame_offset[keep], group=group[keep],
                     kp=kp[keep], t_max=B.t_max, total_frames=B.total_frames)


keep = np.flatnonzero(ms_len <= ops.MAX_TRANSCRIPT)
Ba = sub_batch(keep)
tra = [tr[i] for i in keep]
ep_a = None if pc.endpen is None else pc.endpen[torch.as_tensor(keep, device=dev)].contiguous()
off = np.concatenate([[0], np.cumsum([len(x) for x in tra])]).astype(np.int64)
ws = torch.empty(ops.align_workspace_bytes(Ba, off), dtype=torch.uint8, device=dev)


def align():
    return ops.align(Ba, elp, t['trans'], t['init'], t['len'], tra, endpen=ep_a, ws=ws, want_labels=False)


# the expanded lattice of the videos with M <= 32: one parameter group per video
small = np.flatnonzero(ms_len <= 32)
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
        g, ids, M = int(group[i]), tr[i], len(tr[i])
        o = int(B.frame_offset[i])
        e2[offs[j]:offs[j] + lengths[j], :M] = elp[o:o + int(lengths[j])][:, torch.as_tensor(ids, device=dev)]
        l2[j, :, :M] = lh[g][:, ids]
        i2[j, 0] = ih[g, ids[0]]
        for m in range(1, M):
            t2[j, m, m - 1] = th[g, ids[m], ids[m - 1]]
        p2[j, M - 1] = 0.0 if eh is None else eh[i, ids[-1]]
    Bl = ops.Batch(lengths, ms_len[small], K, c_max=cm, frame_offset=offs, group=np.arange(n, dtype=np.int32), kp=kp[small],
                   t_max=int(lengths.max()), total_frames=int(lengths.sum()))
    lat = (Bl, e2) + tuple(torch.from_numpy(x).to(dev) for x in (t2, i2, l2, p2))

out = align()
torch.cuda.synchronize()
ops.check_decoded(Ba, out)
same = bool(torch.equal(out['best'], vit['best'][torch.as_tensor(keep, device=dev)])
            and torch.equal(out['spans'], vit['spans'][torch.as_tensor(keep, device=dev)]))
same_lat = None
if lat is not None:
    lv = viterbi(*lat)
    torch.cuda.synchronize()
    same_lat = bool(torch.equal(lv['best'], vit['best'][torch.as_tensor(small, device=dev)]))
ms_a, ms_v, ms_l = [], [], []
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    align()
    e[1].record()
    viterbi(B, elp, t['trans'], t['init'], t['len'], pc.endpen)
    e[2].record()
    if lat is not None:
        viterbi(*lat)
    e[3].record()
    torch.cuda.synchronize()
    ms_a.append(e[0].elapsed_time(e[1]))
    ms_v.append(e[1].elapsed_time(e[2]))
    ms_l.append(e[2].elapsed_time(e[3]))
line = ('%s: %d videos, %d frames, longest %d; transcripts: median %d, longest %d entries, %d videos aligned, %d with <= 32 '
      'entries (%d frames); align call %.3f ms, viterbi call %.3f ms, viterbi on the expanded lattices of the <= 32-entry '
      'videos %.3f ms (medians of 5); align == viterbi: %s; expanded lattice == viterbi: %s'
      % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms_len)), int(ms_len.max()), keep.size,
         small.size, int(B.lengths[small].sum()) if small.size else 0, float(np.median(ms_a)), float(np.median(ms_v)),
         float(np.median(ms_l)), same, same_lat))
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
