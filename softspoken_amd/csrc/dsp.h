// Device helpers shared by the front-end kernels (frontend.hip) and the separation kernels (separate.hip): complex arithmetic, the
// 16-point forward DFT, and the PCM sample decode.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ss {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// forward radix-4 butterfly, W4 = -i
__device__ __forceinline__ void radix4(float2 x0, float2 x1, float2 x2, float2 x3, float2& y0, float2& y1, float2& y2, float2& y3) {
    const float2 s02 = cadd(x0, x2), d02 = csub(x0, x2), s13 = cadd(x1, x3), d13 = csub(x1, x3);
    y0 = cadd(s02, s13);
    y2 = csub(s02, s13);
    y1 = make_float2(d02.x + d13.y, d02.y - d13.x);   // d02 - i d13
    y3 = make_float2(d02.x - d13.y, d02.y + d13.x);   // d02 + i d13
}

// 16-point forward DFT in registers, natural order in and out (4 x 4 Cooley-Tukey).
__device__ __forceinline__ void fft16(float2 (&v)[16]) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
    float2 t[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) radix4(v[j], v[j + 4], v[j + 8], v[j + 12], t[j][0], t[j][1], t[j][2], t[j][3]);
    // twiddles W16^(j b)
    t[1][1] = cmul(t[1][1], make_float2(C1, -S1));
    t[1][2] = cmul(t[1][2], make_float2(R2, -R2));
    t[1][3] = cmul(t[1][3], make_float2(S1, -C1));
    t[2][1] = cmul(t[2][1], make_float2(R2, -R2));
    t[2][2] = make_float2(t[2][2].y, -t[2][2].x);                 // W16^4 = -i
    t[2][3] = cmul(t[2][3], make_float2(-R2, -R2));
    t[3][1] = cmul(t[3][1], make_float2(S1, -C1));
    t[3][2] = cmul(t[3][2], make_float2(-R2, -R2));
    t[3][3] = cmul(t[3][3], make_float2(-C1, S1));               // W16^9
#pragma unroll
    for (int b = 0; b < 4; ++b) radix4(t[0][b], t[1][b], t[2][b], t[3][b], v[b], v[b + 4], v[b + 8], v[b + 12]);
}

// PCM -> float32: libsndfile's float conversion (x / 2^(bits-1); unsigned 8-bit is offset by 128); idx counts samples (frame * channels
// + channel), format is enum ss_pcm_format
__device__ __forceinline__ float decode_sample(const unsigned char* p, int format, int64_t idx) {
    switch (format) {
        case 1: return ((float)p[idx] - 128.0f) / 128.0f;
        case 2: return (float)((const short*)p)[idx] / 32768.0f;
        case 3: {
            const unsigned char* b = p + idx * 3;
            int v = (int)b[0] | ((int)b[1] << 8) | ((int)b[2] << 16);
            if (v & 0x800000) v -= 0x1000000;
            return (float)v / 8388608.0f;
        }
        case 4: return (float)((double)((const int*)p)[idx] / 2147483648.0);
        case 5: return ((const float*)p)[idx];
        case 6: return (float)((const double*)p)[idx];
        // AIFF / AIFF-C: big-endian samples, 8-bit ones signed; the same float conversion
        case 7: return (float)(signed char)p[idx] / 128.0f;
        case 8: { const unsigned char* b = p + idx * 2; return (float)(short)((unsigned)b[0] << 8 | b[1]) / 32768.0f; }
        case 9: {
            const unsigned char* b = p + idx * 3;
            int v = (int)b[2] | ((int)b[1] << 8) | ((int)b[0] << 16);
            if (v & 0x800000) v -= 0x1000000;
            return (float)v / 8388608.0f;
        }
        case 10: return (float)((double)(int)__builtin_bswap32(((const uint32_t*)p)[idx]) / 2147483648.0);
        case 11: return __builtin_bit_cast(float, __builtin_bswap32(((const uint32_t*)p)[idx]));
        default: return (float)__builtin_bit_cast(double, __builtin_bswap64(((const uint64_t*)p)[idx]));
    }
}

// float32 -> an integer sample of S = 2^(bits-1) steps per unit (decode_sample's own scale, so a decoded 8-, 16- or 24-bit sample comes
// back as itself): the float32 product y * S -- exact, S being a power of two -- rounded to nearest even, saturated to [-S, S - 1]; a
// NaN gives 0.  hi = S - 1.
__device__ __forceinline__ int quantize_sample(float y, float S, int hi) {
    const float q = rintf(y * S);
    if (!(q == q)) return 0;
    if (q >= S) return hi;
    if (q <= -S) return -hi - 1;
    return (int)q;
}

// float32 -> PCM, the inverse of decode_sample (include/softspoken.h "source output"): sample idx of `p` in `format`.  The integer formats
// store quantize_sample (U8 offset by 128), F32 y's bits, F64 (double)y; 7-12 the same value with its bytes reversed.  24-bit samples are
// three byte stores; every other store is one aligned word of the sample's size (p aligned to it).
__device__ __forceinline__ void encode_sample(unsigned char* p, int format, int64_t idx, float y) {
    switch (format) {
        case 1: p[idx] = (unsigned char)(quantize_sample(y, 128.0f, 127) + 128); break;
        case 2: ((short*)p)[idx] = (short)quantize_sample(y, 32768.0f, 32767); break;
        case 3: {
            const unsigned v = (unsigned)quantize_sample(y, 8388608.0f, 8388607);
            unsigned char* b = p + idx * 3;
            b[0] = (unsigned char)v; b[1] = (unsigned char)(v >> 8); b[2] = (unsigned char)(v >> 16);
            break;
        }
        case 4: ((int*)p)[idx] = quantize_sample(y, 2147483648.0f, 2147483647); break;
        case 5: ((float*)p)[idx] = y; break;
        case 6: ((double*)p)[idx] = (double)y; break;
        case 7: p[idx] = (unsigned char)quantize_sample(y, 128.0f, 127); break;
        case 8: ((unsigned short*)p)[idx] = __builtin_bswap16((unsigned short)quantize_sample(y, 32768.0f, 32767)); break;
        case 9: {
            const unsigned v = (unsigned)quantize_sample(y, 8388608.0f, 8388607);
            unsigned char* b = p + idx * 3;
            b[2] = (unsigned char)v; b[1] = (unsigned char)(v >> 8); b[0] = (unsigned char)(v >> 16);
            break;
        }
        case 10: ((uint32_t*)p)[idx] = __builtin_bswap32((uint32_t)quantize_sample(y, 2147483648.0f, 2147483647)); break;
        case 11: ((uint32_t*)p)[idx] = __builtin_bswap32(__builtin_bit_cast(uint32_t, y)); break;
        default: ((uint64_t*)p)[idx] = __builtin_bswap64(__builtin_bit_cast(uint64_t, (double)y)); break;
    }
}

}  // namespace ss
