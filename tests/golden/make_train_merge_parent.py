"""Write tests/golden/train_merge_parent.npz: the parameter gradients of every case of tests/util_train_merge_cases.py on the build in the tree.

Run ONCE, on a GPU, on a build of the commit BEFORE the merge tails of the training operators moved to csrc/partial_merge.h;
tests/test_gpu_train_merge_parent.py then holds every later build to those bits.  Every case runs twice and has to repeat itself.

    python tests/golden/make_train_merge_parent.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import util_train_merge_cases as C      # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "train_merge_parent.npz")
    arrays = {}
    for name in C.CASES:
        first, again = C.run(name), C.run(name)
        for key, t in first.items():
            assert bool(t.isfinite().all()), (name, key)
            assert bool((t == again[key]).all()), (name, key, "not reproducible")
            arrays[f"{name}/{key}"] = t.detach().cpu().contiguous().numpy()
    np.savez(out_path, **arrays)
    print(f"{len(arrays)} gradients of {len(C.CASES)} cases -> {out_path}")


if __name__ == "__main__":
    main()
