#!/usr/bin/env python3
"""Record the C ABI's dispatch answers into dag_dispatch_answers.json: for every `dp_path` pin the tests use and a grid of
(B, T, L, TR), what dsp_dag_pitch_supported (op 0 / 1), dsp_dag_alignment_trace_optional, dsp_dag_max_alpha_blocks_supported and
the two workspace queries return.  Host logic only: no device call.

    python tests/golden/make_dispatch_answers.py [path/to/libdaspeech_hip.so]

The default library is this repository's build (python -m daspeech_amd.build).  The committed file holds the answers of the library
before kernel selection moved into one function per op (capi_dag.hip); tests/test_capi_symbols.py holds the current build to them.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "dag_dispatch_answers.json")

PATHS = (0, 1, 2, 4, 5, 7, 8, 9)
LS = (1, 5, 127, 128, 1030, 1032, 8192, 8196, 9000, 20480, 38400, 40964)
TRS = (1, 7, 32, 33, 64, 65, 100, 128, 129, 1029, 4095)
BTS = ((4, 50), (32, 512))
COLUMNS = ("dp_path", "B", "T", "L", "TR", "pitch_fwd", "pitch_align", "trace_optional", "blocks_supported",
           "workspace_bytes", "alignment_workspace_bytes")


def answers(lib):
    i = ctypes.c_int
    lib.dsp_dag_set_option.argtypes = [ctypes.c_char_p, i]
    for fn in ("dsp_dag_workspace_bytes", "dsp_dag_alignment_workspace_bytes"):
        getattr(lib, fn).restype = ctypes.c_size_t
        getattr(lib, fn).argtypes = [i, i, i, i]
    rows = []
    try:
        for path in PATHS:
            assert lib.dsp_dag_set_option(b"dp_path", path) == 0
            for B, T in BTS:
                for L in LS:
                    for TR in TRS:
                        rows.append([path, B, T, L, TR, lib.dsp_dag_pitch_supported(0, L, TR), lib.dsp_dag_pitch_supported(1, L, TR),
                                     lib.dsp_dag_alignment_trace_optional(L, TR), lib.dsp_dag_max_alpha_blocks_supported(L, TR),
                                     lib.dsp_dag_workspace_bytes(B, T, L, TR), lib.dsp_dag_alignment_workspace_bytes(B, T, L, TR)])
    finally:
        lib.dsp_dag_set_option(b"dp_path", 0)
    return rows


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "daspeech_amd", "lib", "libdaspeech_hip.so")
    rows = answers(ctypes.CDLL(so))
    n = len(TRS)                                      # one line per (dp_path, B, T, L): its row for every TR
    with open(OUT, "w") as f:
        f.write('{"columns": %s,\n "rows": [\n' % json.dumps(COLUMNS))
        f.write(",\n".join(", ".join(json.dumps(r) for r in rows[i:i + n]) for i in range(0, len(rows), n)))
        f.write("\n]}\n")
    print(f"{OUT}: {len(rows)} rows")


if __name__ == "__main__":
    main()
