"""csrc/split_frag.h on the host: the per-tap base + per-step XOR / add + per-tile constant of SplitBFrag gives, for every row, lane chunk,
32-channel group and column tile, the byte offset the K loops used to compute per (step, tile): (row * CH + split_swz(row, 4 c + lk)) * 16.
Compiled with the host C++ compiler (the header has no device-only code outside its one inline-asm line)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#define __device__
#define __forceinline__ inline
#include <stdio.h>
#include "split_frag.h"
using namespace dsp;
template <int CI> long check() {
    using BF = SplitBFrag<CI>;
    constexpr int CH = CI / 8, NC = CI / 32;
    long bad = 0;
    for (int row0 = 0; row0 < 700; ++row0)
        for (int lk = 0; lk < 4; ++lk) {
            const uint32_t tap = split_keep(BF::tap_base(row0, lk));
            for (int c = 0; c < NC; ++c)
                for (int j = 0; j < 8; ++j) {
                    const int row = row0 + 16 * j;
                    const uint32_t want = ((uint32_t)row * CH + (uint32_t)split_swz<CI>(row, c * 4 + lk)) * 16u;
                    bad += want != BF::step(tap, c) + j * BF::TILE_BYTES;
                }
        }
    printf("CI %d: %ld mismatches\n", CI, bad);
    return bad;
}
int main() { return (check<32>() + check<64>() + check<96>() + check<128>() + check<256>() + check<512>()) != 0; }
"""


def test_fragment_addresses_equal_the_per_tile_formula(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "frag.cpp"
    src.write_text(SRC)
    exe = tmp_path / "frag"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "daspeech_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("0 mismatches") == 6, r.stdout
