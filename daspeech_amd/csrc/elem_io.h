// elem_io.h — elements of the three storage dtypes (fp32 / fp16 / bf16) <-> floats: 8-, 16- and 32-byte groups of a templated T, single
// elements of a tensor known by its dtype code, the element size and the dtype dispatch of the host.  Widening is exact, narrowing is one
// __float2half / __float2bfloat16.  Included by common.h; a kernel takes these from here and does not restate them.
#pragma once

namespace dsp {

// bytes per element of a dtype code, 0 for a code that is none of the three
static inline int elem_size(int dtype) { return dtype == DSP_F32 ? 4 : ((dtype == DSP_F16 || dtype == DSP_BF16) ? 2 : 0); }

// `using T = <element type of dtype>; ...` — the _16 form for kernels that exist in the two 16-bit types only
#define DSP_DISPATCH_ELEM(dtype, T, ...)                                  \
    switch (dtype) {                                                      \
        case DSP_F32: { using T = float; __VA_ARGS__; } break;            \
        case DSP_F16: { using T = __half; __VA_ARGS__; } break;           \
        default: { using T = __hip_bfloat16; __VA_ARGS__; } break;        \
    }
#define DSP_DISPATCH_ELEM_16(dtype, T, ...)                               \
    do {                                                                  \
        if ((dtype) == DSP_F16) { using T = __half; __VA_ARGS__; }        \
        else { using T = __hip_bfloat16; __VA_ARGS__; }                   \
    } while (0)

template <typename T> constexpr int elems16 = 16 / (int)sizeof(T);      // elements per 16 bytes

__device__ __forceinline__ uint32_t bits16(__half v) { return (uint32_t)__half_as_ushort(v); }
__device__ __forceinline__ uint32_t bits16(__hip_bfloat16 v) { unsigned short u; __builtin_memcpy(&u, &v, 2); return (uint32_t)u; }

// one 32-bit word <-> its two 16-bit elements as floats
template <typename T> struct Word;
template <> struct Word<__half> {
    static constexpr int PER = 2;
    static __device__ __forceinline__ void unpack(uint32_t w, float* f)
    {
        f[0] = __half2float(__ushort_as_half((unsigned short)(w & 0xffffu)));
        f[1] = __half2float(__ushort_as_half((unsigned short)(w >> 16)));
    }
    static __device__ __forceinline__ uint32_t pack(const float* f) { return bits16(__float2half(f[0])) | (bits16(__float2half(f[1])) << 16); }
};
template <> struct Word<__hip_bfloat16> {
    static constexpr int PER = 2;
    static __device__ __forceinline__ void unpack(uint32_t w, float* f) { f[0] = __uint_as_float(w << 16); f[1] = __uint_as_float(w & 0xffff0000u); }
    static __device__ __forceinline__ uint32_t pack(const float* f) { return bits16(__float2bfloat16(f[0])) | (bits16(__float2bfloat16(f[1])) << 16); }
};

// 16 bytes of a 16-bit type in registers <-> floats (a kernel with a load or store of its own kind, non-temporal for instance, moves the
// uint4 itself).  By value: a reference to memory would be read as four words.
template <typename T> __device__ __forceinline__ void unpack_f(uint4 u, float* f)
{
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) Word<T>::unpack(w[j], f + j * Word<T>::PER);
}
template <typename T> __device__ __forceinline__ uint4 pack_f(const float* f)
{
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = Word<T>::pack(f + j * Word<T>::PER);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// V consecutive elements, 8, 16 or 32 bytes at an address aligned to min(bytes, 16), widened to float / rounded once from float; fp32 moves
// as float4
template <typename T, int V> __device__ __forceinline__ void load_f(const T* __restrict__ p, float (&f)[V])
{
    constexpr int BYTES = V * (int)sizeof(T);
    static_assert((BYTES == 8 && sizeof(T) == 2) || BYTES == 16 || BYTES == 32, "load_f: 8 (16-bit types), 16 or 32 bytes");
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) {
            const float4 v = reinterpret_cast<const float4*>(p)[i];
            f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
        }
    } else if constexpr (BYTES == 8) {
        const uint2 u = *reinterpret_cast<const uint2*>(p);
        Word<T>::unpack(u.x, f); Word<T>::unpack(u.y, f + Word<T>::PER);
    } else {
#pragma unroll
        for (int i = 0; i < BYTES / 16; ++i) unpack_f<T>(reinterpret_cast<const uint4*>(p)[i], f + i * elems16<T>);
    }
}
template <typename T, int V> __device__ __forceinline__ void store_f(T* __restrict__ p, const float (&f)[V])
{
    constexpr int BYTES = V * (int)sizeof(T);
    static_assert((BYTES == 8 && sizeof(T) == 2) || BYTES == 16 || BYTES == 32, "store_f: 8 (16-bit types), 16 or 32 bytes");
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) reinterpret_cast<float4*>(p)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
    } else if constexpr (BYTES == 8) {
        *reinterpret_cast<uint2*>(p) = make_uint2(Word<T>::pack(f), Word<T>::pack(f + Word<T>::PER));
    } else {
#pragma unroll
        for (int i = 0; i < BYTES / 16; ++i) reinterpret_cast<uint4*>(p)[i] = pack_f<T>(f + i * elems16<T>);
    }
}

// element c of a parameter tensor (a norm's gamma / beta, a bias, running buffers and their gradients) in its own dtype code
__device__ __forceinline__ float param_load(const void* p, int dtype, int c)
{
    if (dtype == DSP_F32) return ((const float*)p)[c];
    if (dtype == DSP_F16) return __half2float(((const __half*)p)[c]);
    return __bfloat162float(((const __hip_bfloat16*)p)[c]);
}
__device__ __forceinline__ void param_store(void* p, int dtype, int c, float v)
{
    if (dtype == DSP_F32) ((float*)p)[c] = v;
    else if (dtype == DSP_F16) ((__half*)p)[c] = __float2half(v);
    else ((__hip_bfloat16*)p)[c] = __float2bfloat16(v);
}
// V parameters from element c on, kept in the data dtype T or in fp32 (the fp32 branch spelled out: through load_f<float> its second
// __restrict__ scope changes the schedule of the callers)
template <typename T, int V> __device__ __forceinline__ void param_load_f(const void* __restrict__ p, int pdtype, int c, float (&f)[V])
{
    if (sizeof(T) == 4 || pdtype != DSP_F32) { load_f<T, V>((const T*)p + c, f); return; }
#pragma unroll
    for (int j = 0; j < V / 4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>((const float*)p + c + 4 * j);
        f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w;
    }
}

}  // namespace dsp
