"""Write tests/golden/split_addressing_parent.npz: the outputs (SHA-256, a CRC-32 per 16 rows and 16 samples each) of every case of
tests/test_gpu_split_addressing.py on the build in the tree.

Run ONCE, on a build of the commit BEFORE the fragment addressing of the split-operand loops moved to csrc/split_frag.h; the test then holds every later
build to those bits.  Each case also passes its fp64 bound here, so the file never records a wrong parent.

    python tools/split_addressing_golden.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_gpu_split_addressing as t      # noqa: E402


def main():
    t.test_conv1d_split_cases_reach_the_instances_they_name()
    out_path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    items = []
    for tag, ti in t.CS_IDS:
        out, ref64, ref32, rows = t.run_cs_case(tag, ti)
        t.check_cs_fp64(out, ref64, ref32, rows, f"{tag} T index {ti}")
        items.append((f"{tag}-{ti}", out))
    for C, K, dil in t.UNITS:
        items += t.run_unit_cases(C, K, dil)
    for tag in t.CONVS:
        items += t.run_conv_case(tag)
    keys, shas, samples, crcs = [], [], [], []
    for key, out in items:
        d, s, c = t.digest(out)
        keys.append(key); shas.append(d); samples.append(s); crcs.append(c)
    assert len(set(keys)) == len(keys)
    off = np.concatenate([[0], np.cumsum([len(c) for c in crcs])]).astype(np.int64)
    np.savez(out_path, keys=np.array(keys), sha256=np.array(shas), samples=np.stack(samples).astype(np.float32), crc_offsets=off,
             crc16rows=np.concatenate(crcs).astype(np.uint32))
    print(f"{len(keys)} outputs -> {out_path}")


if __name__ == "__main__":
    main()
