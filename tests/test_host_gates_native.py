"""csrc/host_gates.h on the host, alone: compiled with the host C++ compiler (the header has no HIP include) next to a small main that
supplies dsp::set_error, every gate is walked through its pass case, each of its refusals with the exact message, and the DSP_ENOSPC /
DSP_EINVAL split of the workspace gate.  The pointers are made-up addresses that nothing reads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "host_gates.h"

static char last[512];
namespace dsp {
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(last, sizeof last, fmt, ap); va_end(ap); }
}
using namespace dsp;

static int bad = 0;
static void expect(int line, int rc, int want_rc, const char* want_msg)
{
    if (rc != want_rc || (want_msg && strcmp(last, want_msg))) { printf("line %d: rc %d (want %d), message '%s'\n", line, rc, want_rc, last); ++bad; }
    if (!want_msg && last[0]) { printf("line %d: a passing gate wrote '%s'\n", line, last); ++bad; }
    last[0] = 0;
}
#define EXPECT(call, rc, msg) expect(__LINE__, (call), (rc), (msg))

static void* at(uintptr_t a) { return (void*)a; }
static int through(int rc) { DSP_GATE(rc); return 7; }

int main()
{
    // a16
    const size_t in[] = {0, 1, 15, 16, 17, 31, 32, ((size_t)1 << 40) + 1}, out[] = {0, 16, 16, 16, 32, 32, 32, ((size_t)1 << 40) + 16};
    for (int i = 0; i < 8; ++i) bad += a16(in[i]) != out[i];
    // on16: every position of the odd pointer, null pointers, mixed pointer types
    const float* f = (const float*)at(0x1000);
    const unsigned char* m = (const unsigned char*)at(0x2010);
    bad += !on16(at(0x1000)) + !on16(f, m, at(0), (void*)nullptr) + on16(at(0x1002)) + on16(at(0x1008)) + on16(f, m, at(0x3001)) + on16(at(0x3004), f, m) +
           on16(f, at(0x300f), m);
    for (uintptr_t o = 1; o < 16; ++o) bad += on16(f, at(0x4000 + o));
    EXPECT(tensors16_gate("op", f, m, at(0)), DSP_OK, nullptr);
    EXPECT(tensors16_gate("op", f, at(0x1002), m), DSP_EINVAL, "op: tensors must be 16-byte aligned");
    // rng_state: null and 8-byte aligned pass
    EXPECT(rng_state_gate("op", nullptr), DSP_OK, nullptr);
    EXPECT(rng_state_gate("op", (const uint64_t*)at(0x1008)), DSP_OK, nullptr);
    EXPECT(rng_state_gate("op_state", (const uint64_t*)at(0x1004)), DSP_EINVAL, "op_state: rng_state must be 8-byte aligned");
    EXPECT(rng_state_gate("op_state", (const uint64_t*)at(0x1001)), DSP_EINVAL, "op_state: rng_state must be 8-byte aligned");
    // workspace: enough, exactly enough, nothing needed; short is ENOSPC only for a usable pointer
    const char* msg = "op: workspace of dsp_op_workspace_bytes(1, ...) bytes (16-byte aligned) needed";
    EXPECT(workspace_gate("op", at(0x1000), 64, 48, "dsp_op_workspace_bytes(1, ...)"), DSP_OK, nullptr);
    EXPECT(workspace_gate("op", at(0x1000), 48, 48, "dsp_op_workspace_bytes(1, ...)"), DSP_OK, nullptr);
    EXPECT(workspace_gate("op", at(0x1000), 0, 0, "dsp_op_workspace_bytes(1, ...)"), DSP_OK, nullptr);
    EXPECT(workspace_gate("op", at(0x1000), 47, 48, "dsp_op_workspace_bytes(1, ...)"), DSP_ENOSPC, msg);
    EXPECT(workspace_gate("op", at(0x1000), 0, 48, "dsp_op_workspace_bytes(1, ...)"), DSP_ENOSPC, msg);
    EXPECT(workspace_gate("op", nullptr, 64, 48, "dsp_op_workspace_bytes(1, ...)"), DSP_EINVAL, msg);
    EXPECT(workspace_gate("op", nullptr, 0, 0, "dsp_op_workspace_bytes(1, ...)"), DSP_EINVAL, msg);
    EXPECT(workspace_gate("op", at(0x1008), 64, 48, "dsp_op_workspace_bytes(1, ...)"), DSP_EINVAL, msg);
    EXPECT(workspace_gate("op", at(0x1002), 0, 48, "dsp_op_workspace_bytes(1, ...)"), DSP_EINVAL, msg);
    // alias: null outputs are not asked for, null inputs match nothing; an input is reported before a second output
    const void* ins[] = {at(0x1000), at(0x2000), nullptr};
    void* ok[] = {at(0x3000), nullptr, at(0x4000), nullptr};
    EXPECT(alias_gate("op", ok, 4, ins, 3, "an output aliases an input", "two outputs alias"), DSP_OK, nullptr);
    EXPECT(alias_gate("op", ok, 0, ins, 0, "a", "b"), DSP_OK, nullptr);
    void* o_in[] = {at(0x3000), nullptr, at(0x2000)};
    EXPECT(alias_gate("op", o_in, 3, ins, 3, "an output aliases an input or the workspace", "two outputs alias"), DSP_EINVAL,
           "op: an output aliases an input or the workspace");
    void* o_out[] = {at(0x3000), nullptr, at(0x4000), at(0x3000)};
    EXPECT(alias_gate("op", o_out, 4, ins, 3, "an output aliases an input", "two outputs alias"), DSP_EINVAL, "op: two outputs alias");
    void* o_both[] = {at(0x3000), at(0x3000), at(0x1000)};         // outs[0]: no input, then outs[1] — reported as two outputs
    EXPECT(alias_gate("op", o_both, 3, ins, 3, "an output aliases an input", "two outputs alias"), DSP_EINVAL, "op: two outputs alias");
    void* o_first[] = {at(0x1000), at(0x1000)};                    // outs[0] is an input: that is what is reported
    EXPECT(alias_gate("op", o_first, 2, ins, 3, "an output aliases an input", "two outputs alias"), DSP_EINVAL, "op: an output aliases an input");
    void* o_last[] = {at(0x3000), at(0x5000)};
    EXPECT(alias_gate("op", o_last, 2, ins, 2, "in", "out"), DSP_OK, nullptr);
    // DSP_GATE leaves with a refusal and goes on after a pass
    bad += through(DSP_OK) != 7;
    bad += through(DSP_EINVAL) != DSP_EINVAL;
    bad += through(DSP_ENOSPC) != DSP_ENOSPC;
    printf("%d mismatches\n", bad);
    return bad != 0;
}
"""


def test_every_gate_passes_and_refuses_as_written(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "gates.cpp"
    src.write_text(SRC)
    exe = tmp_path / "gates"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "daspeech_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 mismatches", r.stdout + r.stderr
