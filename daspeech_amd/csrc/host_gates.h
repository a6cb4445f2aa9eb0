// host_gates.h — the argument gates that the C entries of the training operators share (csrc/*_train.hip): the 16-byte round-up of a
// workspace piece, "these pointers are on the 16-byte grid", and the refusals whose text is the same at every site — a misaligned
// rng_state, a missing / short / misaligned workspace (DSP_ENOSPC for a usable pointer that is too short, DSP_EINVAL otherwise) and the
// "no output aliases an input, no two outputs alias" loop.  A gate returns DSP_OK or its refusal with dsp_last_error() set; an entry calls
// them in the order in which it reports its faults.  A gate whose message belongs to one entry stays at that entry.
// Host only: no HIP include, compiles with a plain C++ compiler (tests/test_host_gates_native.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/daspeech_dag.h"

namespace dsp {

void set_error(const char* fmt, ...);

// leave the entry with a gate's refusal
#define DSP_GATE(gate)                      \
    do {                                    \
        const int refused_ = (gate);        \
        if (refused_) return refused_;      \
    } while (0)

static inline size_t a16(size_t n) { return (n + 15) & ~(size_t)15; }

// every pointer on the 16-byte grid; a null pointer is on it
template <typename... P> static inline bool on16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }

template <typename... P> static inline int tensors16_gate(const char* who, const P*... p)
{
    if (on16(p...)) return DSP_OK;
    set_error("%s: tensors must be 16-byte aligned", who);
    return DSP_EINVAL;
}

static inline int rng_state_gate(const char* who, const uint64_t* p)
{
    if (((uintptr_t)p & 7) == 0) return DSP_OK;
    set_error("%s: rng_state must be 8-byte aligned", who);
    return DSP_EINVAL;
}

// asked: how the message names the size, the entry's workspace question
static inline int workspace_gate(const char* who, const void* ws, size_t have, size_t need, const char* asked)
{
    const bool usable = ws && on16(ws);
    if (usable && have >= need) return DSP_OK;
    set_error("%s: workspace of %s bytes (16-byte aligned) needed", who, asked);
    return usable ? DSP_ENOSPC : DSP_EINVAL;
}

// no output (null ones are not asked for) is an input, no two outputs are the same; reported in the order of outs
static inline int alias_gate(const char* who, void* const* outs, int n_outs, const void* const* ins, int n_ins, const char* out_is_in,
                             const char* out_is_out)
{
    for (int a = 0; a < n_outs; ++a) {
        if (!outs[a]) continue;
        for (int i = 0; i < n_ins; ++i)
            if (outs[a] == ins[i]) { set_error("%s: %s", who, out_is_in); return DSP_EINVAL; }
        for (int c = a + 1; c < n_outs; ++c)
            if (outs[a] == outs[c]) { set_error("%s: %s", who, out_is_out); return DSP_EINVAL; }
    }
    return DSP_OK;
}

}  // namespace dsp
