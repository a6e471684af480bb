"""Golden table of the host API's size and offset queries: what a build of libsmmdp.so returns, byte for byte.

    python tests/golden/make_golden_api_layout.py [path/to/libsmmdp.so]   ->  tests/golden/api_layout.json   (committed)

The queries are host arithmetic (no GPU).  The committed table was made from the build in front of the refactor that gave
smm_api.hip one carving helper and one statement of each layout; tests/test_api_layout_host.py holds every later build to it.
Each row keeps its inputs, so the test replays the rows and needs nothing from this file but ``measure``.
"""
import ctypes
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "api_layout.json")
NO_EOS = 1
MAX_TRANSCRIPT = 256


class Shape(ctypes.Structure):
    _fields_ = [("b", ctypes.c_int32), ("d", ctypes.c_int32), ("n_groups", ctypes.c_int32), ("c_max", ctypes.c_int32),
                ("k_rows", ctypes.c_int32), ("t_max", ctypes.c_int32), ("flags", ctypes.c_int32), ("total_frames", ctypes.c_int64)]


def open_lib(path):
    lib = ctypes.CDLL(path)
    for name in ("smm_workspace_bytes", "smm_error_word_offset", "smm_kbest_workspace_bytes", "smm_mbr_workspace_bytes",
                 "smm_align_workspace_bytes", "smm_entropy_bwd_scratch_bytes", "smm_dense_workspace_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
    lib.smm_dense_workspace_bytes.argtypes = [ctypes.c_int32] * 4
    return lib


def measure(lib, row):
    """The queries' answers for one row of inputs: {query name: bytes}."""
    if row["kind"] == "dense":
        return {"dense": int(lib.smm_dense_workspace_bytes(row["b"], row["n1"], row["k"], row["c"]))}
    lengths = np.asarray(row["lengths"], np.int64)
    toff = np.asarray(row["toff"], np.int64)
    s = Shape(len(lengths), 0, row["n_groups"], row["c_max"], row["k_rows"], row["t_max"], row["flags"], row["total_frames"])
    sp, lp, tp = ctypes.byref(s), ctypes.c_void_p(lengths.ctypes.data), ctypes.c_void_p(toff.ctypes.data)
    return {"workspace": int(lib.smm_workspace_bytes(sp, lp)),
            "error_word_offset": int(lib.smm_error_word_offset(sp)),
            "kbest": int(lib.smm_kbest_workspace_bytes(sp, lp, ctypes.c_int32(row["k"]))),
            "mbr": int(lib.smm_mbr_workspace_bytes(sp, lp)),
            "align": int(lib.smm_align_workspace_bytes(sp, lp, tp)),
            "entropy_bwd_scratch": int(lib.smm_entropy_bwd_scratch_bytes(sp, lp))}


def _row(lengths, n_groups, c_max, k_rows, k, m, flags=0, t_max=None, toff=None, zero=()):
    """m: transcript entries per video.  zero: the queries that must answer 0 for this row."""
    lengths = [int(t) for t in lengths]
    t_max = max(max(lengths), 1) if t_max is None else t_max
    if toff is None:
        toff = [m * i for i in range(len(lengths) + 1)]
    return dict(kind="smm", lengths=lengths, n_groups=n_groups, c_max=c_max, k_rows=k_rows, t_max=t_max, flags=flags,
                total_frames=len(lengths) * t_max, k=k, toff=[int(v) for v in toff], zero=list(zero))


def rows():
    out = []
    ragged = lambda b: [(5 * i) % 11 + 1 for i in range(b)]          # video 0 has T = 1
    grid = itertools.product((1, 2, 7, 65), (1, 3), (1, 3, 32), (2, 4, 1024))
    for n, (b, g, c, kr) in enumerate(grid):
        lengths = ragged(b) if (b > 1 or n % 2) else [9]
        out.append(_row(lengths, g, c, kr, k=(1, 16)[n % 2], m=(1, MAX_TRANSCRIPT)[(n // 2) % 2], flags=NO_EOS if n % 5 == 0 else 0,
                        t_max=max(lengths) + (3 if n % 3 == 0 else 0),
                        zero=("align",) if n % 5 == 0 else ()))
    # transcripts of mixed lengths, offsets that do not start at 0
    out.append(_row(ragged(7), 3, 3, 4, k=16, m=0, toff=[4, 5, 261, 263, 270, 271, 527, 530]))
    # rows that are refused
    every = ("workspace", "kbest", "mbr", "align", "entropy_bwd_scratch")
    sized = ("kbest", "mbr", "align", "entropy_bwd_scratch")        # (smm_workspace_bytes itself does not look at the limits)
    out.append(_row([4, 0, 3], 1, 3, 4, k=4, m=2, t_max=4, zero=every))                   # a length of 0
    out.append(_row([4, 7, 3], 1, 3, 4, k=4, m=2, t_max=6, zero=every))                   # a length above t_max
    out.append(_row([4, 6, 3], 1, 33, 4, k=4, m=2, zero=sized))                           # c_max 33
    out.append(_row([4, 6, 3], 1, 3, 1025, k=4, m=2, zero=sized))                         # k_rows 1025
    out.append(_row([4, 6, 3], 1, 3, 4, k=17, m=2, zero=("kbest",)))                      # k 17
    out.append(_row([4, 6, 3], 1, 3, 4, k=0, m=2, zero=("kbest",)))                       # k 0
    out.append(_row([4, 6, 3], 1, 3, 4, k=4, m=2, flags=NO_EOS, zero=("align",)))         # NO_EOS for align
    out.append(_row([4, 6, 3], 1, 3, 4, k=4, m=0, toff=[0, 2, 1, 3], zero=("align",)))    # non-monotone transcript offsets
    out.append(_row([4, 6, 3], 1, 3, 4, k=4, m=0, toff=[0, 2, 2, 3], zero=("align",)))    # an empty transcript
    out.append(_row([4, 6, 3], 1, 3, 4, k=4, m=0, toff=[0, 2, 259, 260], zero=("align",)))   # 257 entries
    out.append(_row([4, 6, 3], 1, 3, 4, k=4, m=0, toff=[-1, 2, 3, 4], zero=("align",)))   # a negative first offset
    out.append(_row([4, 6, 3], 1, 3, 1, k=4, m=2, zero=every + ("error_word_offset",)))  # k_rows 1: no valid shape
    for b, n1, k, c in itertools.product((1, 2, 7, 65), (1, 5, 33), (1, 4), (1, 3, 32)):
        out.append(dict(kind="dense", b=b, n1=n1, k=k, c=c, zero=[]))
    for bad in ((0, 5, 4, 3), (2, 0, 4, 3), (2, 5, 0, 3), (2, 5, 4, 0)):
        out.append(dict(kind="dense", b=bad[0], n1=bad[1], k=bad[2], c=bad[3], zero=["dense"]))
    return out


def main():
    default = os.path.join(HERE, "..", "..", "action-segmentation_amd", "libsmmdp.so")
    lib = open_lib(sys.argv[1] if len(sys.argv) > 1 else default)
    table = []
    for row in rows():
        got = measure(lib, row)
        for name, v in got.items():
            assert (v == 0) == (name in row["zero"]), (row, name, v)
        table.append(dict(row, out=got))
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in table) + "\n]\n")
    print("%d rows -> %s" % (len(table), OUT))


if __name__ == "__main__":
    main()
