// tts_loss_train.hip — the four TTS losses of the released objective under autograd, gfx950, the masks taken from the lengths
// (DASpeech/criterions/s2s_dag_fastspeech2_loss.py:266-290; include/daspeech_decode.h: dsp_tts_loss_fwd / _bwd).  With F_ = min(F, Fa),
// m_b = min(audio_len[b], F_), s_b = min(src_len[b], N), n_mel = C * sum_b m_b, n_src = sum_b s_b:
//     l1     = sum_{b, f < m_b, c} |feat_out - target| / n_mel   (+ the same sum over feat_post, also / n_mel)
//     dur    = sum_{b, n < s_b} (log_dur_out - log(durations + 1))^2 / n_src         pitch, energy: the same on their own pairs
// fp32 / fp16 / bf16 storage, fp32 arithmetic on the exactly widened inputs, four fp32 results.  No mask tensor, no selection, no host read.
//
// Forward, two launches.  tl_partial_kernel: the mel rows (b, f) of the [B, F_] grid are cut into chunks of DSP_TTSLOSS_CHUNK_ROWS rows, the
// B * N variance elements into chunks of DSP_TTSLOSS_CHUNK_ELEMS; ONE WAVE owns a chunk, each lane adds its share of the chunk's valid terms
// in ascending order in an fp32 register, wave_sum folds the 64 lanes, and lane 0 writes the chunk's partial to its slot of the workspace
// (plain stores; a chunk without a valid row writes 0).  Which terms a lane adds and which slot a chunk owns follow from the shapes, the
// dtype and the alignment alone — never from the lengths, the grid or the schedule.  tl_tail_kernel: one workgroup; thread t adds the
// partials t, t + 256, ... in ascending order, wave_sum, then thread 0 adds the four waves in wave order; the same workgroup sums the
// lengths as integers and writes losses[4] and the two reciprocals.  No float atomics, no hand-off between workgroups inside a launch.
//
// Backward, one launch: a thread owns a 16-byte group of a mel row (or one element on the scalar path) or one variance element, recomputes
// the difference from the saved inputs and writes every element of every gradient asked for — exact zeros outside the lengths.
//
// All of it is row traffic of a few MB: 16-byte accesses per lane where C, the strides and the pointers allow, a scalar path otherwise.
#include "common.h"
#include "host_gates.h"
#include "../../include/daspeech_decode.h"

namespace dsp {

constexpr int TL_ROWS = DSP_TTSLOSS_CHUNK_ROWS;            // mel rows per chunk = per workspace partial
constexpr int TL_ELEMS = DSP_TTSLOSS_CHUNK_ELEMS;          // [B,N] elements per chunk
constexpr int TL_MAX_WG = 1024;                            // 4 waves each
constexpr int TL_TAIL = 256;                               // threads of the tail

__device__ __forceinline__ long tl_len(const void* lens, int len64, int b)
{
    return len64 ? (long)((const int64_t*)lens)[b] : (long)((const int32_t*)lens)[b];
}
__device__ __forceinline__ unsigned tl_clamp(long v, unsigned hi) { return v < 0 ? 0u : (v > (long)hi ? hi : (unsigned)v); }

// a mel tensor as the kernels take it: base, batch stride, row stride (elements); unit column stride
template <typename T> struct Mel {
    const T* p; size_t sb, sr;
    __device__ __forceinline__ const T* row(unsigned b, unsigned f) const { return p + (size_t)b * sb + (size_t)f * sr; }
};

// ---------------------------------------------------------------- forward, first launch: one partial per chunk
template <typename T>
__global__ __launch_bounds__(256) void tl_partial_kernel(Mel<T> fo, Mel<T> fp, Mel<T> tg, const void* __restrict__ alen,
                                                         const T* __restrict__ ld, const T* __restrict__ po, const T* __restrict__ eo,
                                                         const void* __restrict__ dur, const T* __restrict__ pt, const T* __restrict__ et,
                                                         const void* __restrict__ slen, int len64, int dur64, float* __restrict__ part,
                                                         unsigned B, unsigned F_, unsigned C, unsigned N, unsigned nc_mel, unsigned nc_src, bool vec)
{
    constexpr int V = elems16<T>;
    const unsigned lane = threadIdx.x & 63;
    const unsigned R = B * F_, E = B * N;
    float* p_l1 = part;
    float* p_post = part + nc_mel;
    float* p_dur = part + 2 * (size_t)nc_mel;
    float* p_pitch = p_dur + nc_src;
    float* p_energy = p_pitch + nc_src;
    for (unsigned u = blockIdx.x * 4 + (threadIdx.x >> 6); u < nc_mel + nc_src; u += gridDim.x * 4) {
        if (u < nc_mel) {
            const unsigned r0 = u * TL_ROWS;
            float s1 = 0.f, s2 = 0.f;
            if (vec) {
                const unsigned gr = C / V;                                 // 16-byte groups per row
                for (unsigned g = lane; g < TL_ROWS * gr; g += 64) {
                    const unsigned r = r0 + g / gr, c = (g % gr) * V;
                    if (r >= R) break;
                    const unsigned b = r / F_, f = r - b * F_;
                    if (f >= tl_clamp(tl_len(alen, len64, b), F_)) continue;
                    float a[V], t[V];
                    load_f<T, V>(fo.row(b, f) + c, a);
                    load_f<T, V>(tg.row(b, f) + c, t);
#pragma unroll
                    for (int i = 0; i < V; ++i) s1 += fabsf(a[i] - t[i]);
                    if (fp.p) {
                        load_f<T, V>(fp.row(b, f) + c, a);
#pragma unroll
                        for (int i = 0; i < V; ++i) s2 += fabsf(a[i] - t[i]);
                    }
                }
            } else {
                for (unsigned g = lane; g < TL_ROWS * C; g += 64) {
                    const unsigned r = r0 + g / C, c = g % C;
                    if (r >= R) break;
                    const unsigned b = r / F_, f = r - b * F_;
                    if (f >= tl_clamp(tl_len(alen, len64, b), F_)) continue;
                    const float t = to_f(tg.row(b, f)[c]);
                    s1 += fabsf(to_f(fo.row(b, f)[c]) - t);
                    if (fp.p) s2 += fabsf(to_f(fp.row(b, f)[c]) - t);
                }
            }
            s1 = wave_sum(s1); s2 = wave_sum(s2);
            if (lane == 0) { p_l1[u] = s1; p_post[u] = s2; }
        } else {
            const unsigned k = u - nc_mel, e0 = k * TL_ELEMS;
            float sd = 0.f, sp = 0.f, se = 0.f;
            for (unsigned j = lane; j < TL_ELEMS; j += 64) {
                const unsigned e = e0 + j;
                if (e >= E) break;
                const unsigned b = e / N, n = e - b * N;
                if (n >= tl_clamp(tl_len(slen, len64, b), N)) continue;
                const float d = dur64 ? (float)((const int64_t*)dur)[e] : (float)((const int32_t*)dur)[e];
                const float dd = to_f(ld[e]) - logf(d + 1.f);
                const float dp = to_f(po[e]) - to_f(pt[e]);
                const float de = to_f(eo[e]) - to_f(et[e]);
                sd += dd * dd; sp += dp * dp; se += de * de;
            }
            sd = wave_sum(sd); sp = wave_sum(sp); se = wave_sum(se);
            if (lane == 0) { p_dur[k] = sd; p_pitch[k] = sp; p_energy[k] = se; }
        }
    }
}

// ---------------------------------------------------------------- forward, tail: the partials in an order fixed by their index
// sum of v[0..n): thread t takes t, t + TL_TAIL, ... in ascending order, wave_sum, thread 0 adds the waves in wave order (valid in thread 0)
__device__ __forceinline__ float tl_tail_sum(const float* __restrict__ v, unsigned n, float* sh)
{
    float s = 0.f;
    for (unsigned k = threadIdx.x; k < n; k += TL_TAIL) s += v[k];
    s = wave_sum(s);
    __syncthreads();                                                       // sh is free again
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    float r = sh[0];
#pragma unroll
    for (int w = 1; w < TL_TAIL / 64; ++w) r += sh[w];
    return r;
}
__device__ __forceinline__ long long tl_tail_count(const void* __restrict__ lens, int len64, unsigned B, unsigned hi, long long* sh)
{
    long long s = 0;
    for (unsigned b = threadIdx.x; b < B; b += TL_TAIL) s += (long long)tl_clamp(tl_len(lens, len64, (int)b), hi);
    s = lanes_sum<64>(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    long long r = sh[0];
#pragma unroll
    for (int w = 1; w < TL_TAIL / 64; ++w) r += sh[w];
    return r;
}

__global__ __launch_bounds__(TL_TAIL) void tl_tail_kernel(const float* __restrict__ part, const void* __restrict__ alen,
                                                          const void* __restrict__ slen, int len64, bool post, float* __restrict__ losses,
                                                          float* __restrict__ inv_counts, unsigned B, unsigned F_, unsigned C, unsigned N,
                                                          unsigned nc_mel, unsigned nc_src)
{
    __shared__ float shf[TL_TAIL / 64];
    __shared__ long long shi[TL_TAIL / 64];
    const float* p_dur = part + 2 * (size_t)nc_mel;
    const float s_l1 = tl_tail_sum(part, nc_mel, shf);
    const float s_post = post ? tl_tail_sum(part + nc_mel, nc_mel, shf) : 0.f;
    const float s_dur = tl_tail_sum(p_dur, nc_src, shf);
    const float s_pitch = tl_tail_sum(p_dur + nc_src, nc_src, shf);
    const float s_energy = tl_tail_sum(p_dur + 2 * (size_t)nc_src, nc_src, shf);
    const double n_mel = (double)((long long)C * tl_tail_count(alen, len64, B, F_, shi));
    const double n_src = (double)tl_tail_count(slen, len64, B, N, shi);
    if (threadIdx.x) return;
    // the integer counts divide exactly once: (double) sum / (double) count, rounded to fp32; 0 / 0 = NaN as torch's mean of nothing
    float l1 = (float)((double)s_l1 / n_mel);
    if (post) l1 += (float)((double)s_post / n_mel);
    losses[0] = l1;
    losses[1] = (float)((double)s_dur / n_src);
    losses[2] = (float)((double)s_pitch / n_src);
    losses[3] = (float)((double)s_energy / n_src);
    inv_counts[0] = (float)(1.0 / n_mel);
    inv_counts[1] = (float)(1.0 / n_src);
}

// ---------------------------------------------------------------- backward: every element of every gradient asked for
__device__ __forceinline__ float tl_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }     // sign(0) = sign(NaN) = 0

template <typename T>
__global__ __launch_bounds__(256) void tl_bwd_kernel(const float* __restrict__ grad, const float* __restrict__ inv_counts, Mel<T> fo, Mel<T> fp,
                                                     Mel<T> tg, const void* __restrict__ alen, const T* __restrict__ ld,
                                                     const T* __restrict__ po, const T* __restrict__ eo, const void* __restrict__ dur,
                                                     const T* __restrict__ pt, const T* __restrict__ et, const void* __restrict__ slen,
                                                     int len64, int dur64, T* __restrict__ d_fo, T* __restrict__ d_fp, T* __restrict__ d_ld,
                                                     T* __restrict__ d_po, T* __restrict__ d_eo, unsigned F, unsigned F_, unsigned C,
                                                     unsigned N, unsigned n_mel_units, unsigned n_src_units, bool vec)
{
    constexpr int V = elems16<T>;
    const float k_l1 = grad[0] * inv_counts[0];
    const float k_dur = grad[1] * inv_counts[1], k_pitch = grad[2] * inv_counts[1], k_energy = grad[3] * inv_counts[1];
    const unsigned total = n_mel_units + n_src_units;
    for (unsigned u = blockIdx.x * 256 + threadIdx.x; u < total; u += gridDim.x * 256) {
        if (u < n_mel_units) {
            if (vec) {
                const unsigned gr = C / V;
                const unsigned r = u / gr, c = (u - r * gr) * V;           // row of the [B, F] grid of the OUTPUTS
                const unsigned b = r / F, f = r - b * F;
                const bool on = f < tl_clamp(tl_len(alen, len64, b), F_);
                float t[V], a[V], o[V];
                const size_t at = (size_t)r * C + c;
                if (on) load_f<T, V>(tg.row(b, f) + c, t);
                if (d_fo) {
#pragma unroll
                    for (int i = 0; i < V; ++i) o[i] = 0.f;
                    if (on) {
                        load_f<T, V>(fo.row(b, f) + c, a);
#pragma unroll
                        for (int i = 0; i < V; ++i) o[i] = tl_sign(a[i] - t[i]) * k_l1;
                    }
                    store_f<T, V>(d_fo + at, o);
                }
                if (d_fp) {
#pragma unroll
                    for (int i = 0; i < V; ++i) o[i] = 0.f;
                    if (on) {
                        load_f<T, V>(fp.row(b, f) + c, a);
#pragma unroll
                        for (int i = 0; i < V; ++i) o[i] = tl_sign(a[i] - t[i]) * k_l1;
                    }
                    store_f<T, V>(d_fp + at, o);
                }
            } else {
                const unsigned r = u / C, c = u - r * C;
                const unsigned b = r / F, f = r - b * F;
                const bool on = f < tl_clamp(tl_len(alen, len64, b), F_);
                const float t = on ? to_f(tg.row(b, f)[c]) : 0.f;
                if (d_fo) d_fo[u] = from_f<T>(on ? tl_sign(to_f(fo.row(b, f)[c]) - t) * k_l1 : 0.f);
                if (d_fp) d_fp[u] = from_f<T>(on ? tl_sign(to_f(fp.row(b, f)[c]) - t) * k_l1 : 0.f);
            }
        } else {
            const unsigned e = u - n_mel_units;
            const unsigned b = e / N, n = e - b * N;
            const bool on = n < tl_clamp(tl_len(slen, len64, b), N);
            if (d_ld) {
                float v = 0.f;
                if (on) {
                    const float d = dur64 ? (float)((const int64_t*)dur)[e] : (float)((const int32_t*)dur)[e];
                    v = 2.f * (to_f(ld[e]) - logf(d + 1.f)) * k_dur;
                }
                d_ld[e] = from_f<T>(v);
            }
            if (d_po) d_po[e] = from_f<T>(on ? 2.f * (to_f(po[e]) - to_f(pt[e])) * k_pitch : 0.f);
            if (d_eo) d_eo[e] = from_f<T>(on ? 2.f * (to_f(eo[e]) - to_f(et[e])) * k_energy : 0.f);
        }
    }
}

static unsigned tl_chunks(long n, int per) { return n <= 0 ? 0u : (unsigned)((n + per - 1) / per); }
static unsigned tl_grid(unsigned units, unsigned per_wg)
{
    const unsigned g = (units + per_wg - 1) / per_wg;
    return g < 1 ? 1u : (g > (unsigned)TL_MAX_WG ? (unsigned)TL_MAX_WG : g);
}

// the three mel tensors in the 16-byte form: C, every stride and every pointer on the grid of V elements
static bool tl_vec(int es, int C, const void* const* ptrs, const long* strides, int np, int ns)
{
    const int V = 16 / es;
    if (C % V) return false;
    for (int i = 0; i < np; ++i) if ((uintptr_t)ptrs[i] & 15) return false;
    for (int i = 0; i < ns; ++i) if (strides[i] % V) return false;
    return true;
}

// what both entry points check; 1: nothing to do (B == 0), 0: go on, < 0: refused
static int tl_check(const char* who, int dtype, int B, int F, int F_, int C, int N, const long* strides, int ns)
{
    if (!elem_size(dtype)) { set_error("%s: dtype code %d (fp32, fp16 or bf16)", who, dtype); return DSP_EINVAL; }
    if (B < 0 || F < 1 || F_ < 1 || F_ > F || C < 1 || N < 1 || (double)B * F * C > DSP_TTSLOSS_MAX_ELEMS || (double)B * N > DSP_TTSLOSS_MAX_ELEMS) {
        set_error("%s: bad sizes B=%d F=%d F_=%d C=%d N=%d (B >= 0, 1 <= F_ <= F, C >= 1, N >= 1, B*F*C and B*N at most %ld)", who, B, F, F_, C, N,
                  (long)DSP_TTSLOSS_MAX_ELEMS);
        return DSP_EINVAL;
    }
    for (int i = 0; i < ns; ++i)
        if (strides[i] < 0) { set_error("%s: negative stride %ld", who, strides[i]); return DSP_EINVAL; }
    return B == 0 ? 1 : 0;
}

}  // namespace dsp

using namespace dsp;

extern "C" size_t dsp_tts_loss_workspace_bytes(int B, int F_, int N)
{
    if (B <= 0) return 0;
    const size_t n = 2 * (size_t)tl_chunks(F_ > 0 ? (long)B * F_ : 0, TL_ROWS) + 3 * (size_t)tl_chunks(N > 0 ? (long)B * N : 0, TL_ELEMS);
    return a16(n * sizeof(float));
}

extern "C" int dsp_tts_loss_fwd(const void* feat_out, long fo_sb, long fo_sr, const void* feat_post, long fp_sb, long fp_sr,
                                const void* target, long tg_sb, long tg_sr, const void* audio_lens, const void* log_dur_out,
                                const void* pitch_out, const void* energy_out, const void* durations, const void* pitches, const void* energies,
                                const void* src_lens, int len64, int dur64, float* losses, float* inv_counts, void* workspace,
                                size_t workspace_bytes, int dtype, int B, int F_, int C, int N, dsp_stream_t stream)
{
    const char* who = "tts_loss_fwd";
    const long strides[6] = {fo_sb, fo_sr, feat_post ? fp_sb : 0, feat_post ? fp_sr : 0, tg_sb, tg_sr};
    const int rc = tl_check(who, dtype, B, F_, F_, C, N, strides, 6);
    if (rc) return rc < 0 ? rc : DSP_OK;
    const void* in[11] = {feat_out, target, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies, src_lens, feat_post};
    for (int i = 0; i < 10; ++i)
        if (!in[i]) { set_error("%s: null pointer (input %d)", who, i); return DSP_EINVAL; }
    if (!losses || !inv_counts) { set_error("%s: null pointer (losses, inv_counts)", who); return DSP_EINVAL; }
    for (int i = 0; i < 11; ++i)
        if (in[i] && (in[i] == (const void*)losses || in[i] == (const void*)inv_counts || in[i] == workspace)) {
            set_error("%s: an output or the workspace aliases input %d", who, i); return DSP_EINVAL;
        }
    if ((const void*)losses == workspace || (const void*)inv_counts == workspace || losses == inv_counts) {
        set_error("%s: losses, inv_counts and the workspace alias", who); return DSP_EINVAL;
    }
    const int es = elem_size(dtype);
    const uintptr_t grid_bits = (uintptr_t)feat_out | (uintptr_t)feat_post | (uintptr_t)target | (uintptr_t)log_dur_out | (uintptr_t)pitch_out |
                                (uintptr_t)energy_out | (uintptr_t)pitches | (uintptr_t)energies;
    if ((grid_bits & (uintptr_t)(es - 1)) || (((uintptr_t)losses | (uintptr_t)inv_counts) & 3) ||
        (((uintptr_t)audio_lens | (uintptr_t)src_lens) & (len64 ? 7 : 3)) || ((uintptr_t)durations & (dur64 ? 7 : 3))) {
        set_error("%s: a pointer is off the grid of its element type", who); return DSP_EINVAL;
    }
    if (!workspace || !on16(workspace) || workspace_bytes < dsp_tts_loss_workspace_bytes(B, F_, N)) {
        set_error("%s: workspace of %zu bytes (16-byte aligned) needed, see dsp_tts_loss_workspace_bytes", who, dsp_tts_loss_workspace_bytes(B, F_, N));
        return workspace && on16(workspace) ? DSP_ENOSPC : DSP_EINVAL;
    }
    const void* vp[3] = {feat_out, target, feat_post};
    const bool vec = tl_vec(es, C, vp, strides, 3, 6);
    const unsigned nc_mel = tl_chunks((long)B * F_, TL_ROWS), nc_src = tl_chunks((long)B * N, TL_ELEMS);
    hipStream_t st = as_stream(stream);
    DSP_DISPATCH_ELEM(dtype, T, {
        const Mel<T> fo{(const T*)feat_out, (size_t)fo_sb, (size_t)fo_sr}, fp{(const T*)feat_post, (size_t)strides[2], (size_t)strides[3]},
            tg{(const T*)target, (size_t)tg_sb, (size_t)tg_sr};
        hipLaunchKernelGGL(tl_partial_kernel<T>, dim3(tl_grid(nc_mel + nc_src, 4)), dim3(256), 0, st, fo, fp, tg, audio_lens,
                           (const T*)log_dur_out, (const T*)pitch_out, (const T*)energy_out, durations, (const T*)pitches, (const T*)energies,
                           src_lens, len64, dur64, (float*)workspace, (unsigned)B, (unsigned)F_, (unsigned)C, (unsigned)N, nc_mel, nc_src, vec);
    });
    hipLaunchKernelGGL(tl_tail_kernel, dim3(1), dim3(TL_TAIL), 0, st, (const float*)workspace, audio_lens, src_lens, len64, feat_post != nullptr,
                       losses, inv_counts, (unsigned)B, (unsigned)F_, (unsigned)C, (unsigned)N, nc_mel, nc_src);
    return check_launch(who);
}

extern "C" int dsp_tts_loss_bwd(const float* grad_losses, const float* inv_counts, const void* feat_out, long fo_sb, long fo_sr,
                                const void* feat_post, long fp_sb, long fp_sr, const void* target, long tg_sb, long tg_sr,
                                const void* audio_lens, const void* log_dur_out, const void* pitch_out, const void* energy_out,
                                const void* durations, const void* pitches, const void* energies, const void* src_lens, int len64, int dur64,
                                void* d_feat_out, void* d_feat_post, void* d_log_dur, void* d_pitch, void* d_energy, int dtype, int B, int F,
                                int F_, int C, int N, dsp_stream_t stream)
{
    const char* who = "tts_loss_bwd";
    const long strides[6] = {fo_sb, fo_sr, feat_post ? fp_sb : 0, feat_post ? fp_sr : 0, tg_sb, tg_sr};
    const int rc = tl_check(who, dtype, B, F, F_, C, N, strides, 6);
    if (rc) return rc < 0 ? rc : DSP_OK;
    void* out[5] = {d_feat_out, d_feat_post, d_log_dur, d_pitch, d_energy};
    if (!d_feat_out && !d_feat_post && !d_log_dur && !d_pitch && !d_energy) return DSP_OK;
    const void* in[13] = {grad_losses, inv_counts, feat_out, target, audio_lens, log_dur_out, pitch_out, energy_out, durations, pitches, energies,
                          src_lens, feat_post};
    for (int i = 0; i < 12; ++i)
        if (!in[i]) { set_error("%s: null pointer (input %d)", who, i); return DSP_EINVAL; }
    if (d_feat_post && !feat_post) { set_error("%s: d_feat_post without feat_post", who); return DSP_EINVAL; }
    for (int o = 0; o < 5; ++o) {
        if (!out[o]) continue;
        for (int i = 0; i < 13; ++i)
            if (out[o] == in[i]) { set_error("%s: gradient %d aliases input %d", who, o, i); return DSP_EINVAL; }
        for (int p = 0; p < o; ++p)
            if (out[o] == out[p]) { set_error("%s: gradients %d and %d alias", who, p, o); return DSP_EINVAL; }
    }
    const int es = elem_size(dtype);
    uintptr_t grid_bits = (uintptr_t)feat_out | (uintptr_t)feat_post | (uintptr_t)target | (uintptr_t)log_dur_out | (uintptr_t)pitch_out |
                          (uintptr_t)energy_out | (uintptr_t)pitches | (uintptr_t)energies;
    for (int o = 0; o < 5; ++o) grid_bits |= (uintptr_t)out[o];
    if ((grid_bits & (uintptr_t)(es - 1)) || (((uintptr_t)grad_losses | (uintptr_t)inv_counts) & 3) ||
        (((uintptr_t)audio_lens | (uintptr_t)src_lens) & (len64 ? 7 : 3)) || ((uintptr_t)durations & (dur64 ? 7 : 3))) {
        set_error("%s: a pointer is off the grid of its element type", who); return DSP_EINVAL;
    }
    const bool mel = d_feat_out || d_feat_post, src = d_log_dur || d_pitch || d_energy;
    const void* vp[5] = {feat_out, target, feat_post, d_feat_out, d_feat_post};
    const bool vec = tl_vec(es, C, vp, strides, 5, 6);
    const unsigned n_mel_units = mel ? (unsigned)((size_t)B * F * (vec ? C / (16 / es) : C)) : 0u;
    const unsigned n_src_units = src ? (unsigned)B * (unsigned)N : 0u;
    DSP_DISPATCH_ELEM(dtype, T, {
        const Mel<T> fo{(const T*)feat_out, (size_t)fo_sb, (size_t)fo_sr}, fp{(const T*)feat_post, (size_t)strides[2], (size_t)strides[3]},
            tg{(const T*)target, (size_t)tg_sb, (size_t)tg_sr};
        hipLaunchKernelGGL(tl_bwd_kernel<T>, dim3(tl_grid(n_mel_units + n_src_units, 256)), dim3(256), 0, as_stream(stream), grad_losses, inv_counts,
                           fo, fp, tg, audio_lens, (const T*)log_dur_out, (const T*)pitch_out, (const T*)energy_out, durations, (const T*)pitches,
                           (const T*)energies, src_lens, len64, dur64, (T*)d_feat_out, (T*)d_feat_post, (T*)d_log_dur, (T*)d_pitch, (T*)d_energy,
                           (unsigned)F, (unsigned)F_, (unsigned)C, (unsigned)N, n_mel_units, n_src_units, vec);
    });
    return check_launch(who);
}
