"""Write tests/golden/train_entry_refusals.json: what the build in the tree answers to every call of tests/util_train_entry_refusal_calls.py,
as [entry, case, rc, message] (the message is dsp_last_error() after a refusal, "" after DSP_OK).  No GPU is needed: every call is answered by
the argument gates.

Run ONCE, on a build of the commit BEFORE the gates moved to csrc/host_gates.h; tests/test_train_entry_refusals.py then holds every later
build to those return codes and those message bytes.

    python tests/golden/make_train_entry_refusals.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from daspeech_amd import _lib                            # noqa: E402
from tests import util_train_entry_refusal_calls as U    # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "train_entry_refusals.json")
    lib = _lib.load()
    rows = []
    for sym, case, ok, args in U.calls():
        rc = getattr(lib, sym)(*args)
        if ok:
            assert rc == 0, (sym, case, rc)
            rows.append([sym, case, 0, ""])
        else:
            assert rc < 0, (sym, case, rc, "this call is not refused: it must not be in the table")
            rows.append([sym, case, rc, lib.dsp_last_error().decode("utf-8")])
    with open(out_path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} calls of {len(U.ENTRIES)} entries (and their _state twins) -> {out_path}")


if __name__ == "__main__":
    main()
