// q4_0_host_check.cpp -- a stand-alone run of the Q4_0 host code (include/gguf_quant.h) for the
// sanitizers: the block producer, the dequantizer and gq_cpu_mmq type 6 on exactly sized heap
// buffers (the last block ends its allocation), type 6 compared bit for bit with type 0 on the
// widened blocks.  Never loaded into Python.  From the repository root:
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/q4_0_host_check.cpp gguf-triton-kernel_amd/csrc/quant/gguf_quant.cpp \
//       gguf-triton-kernel_amd/csrc/quant/gguf_cpu_mmq.cpp -pthread -o q4_0_host_check && ./q4_0_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gguf_quant.h"

static uint32_t g_state = 12345u;
static float rnd() // uniform in (-1, 1)
{
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) / 8388608.f - 1.f;
}

int main()
{
    const int64_t M = 37, N = 5, K = 1120, nb = K / 32; // K % 256 != 0, K % 64 == 32
    // heap buffers of the exact sizes: an access past the last block is an ASan report
    float *x = (float *)malloc(sizeof(float) * M * K);
    for (int64_t i = 0; i < M * K; ++i) x[i] = rnd();
    for (int64_t i = 0; i < 32; ++i) x[i] = 0.f; // an all-zero block
    uint8_t *q4 = (uint8_t *)malloc(M * nb * 18);
    gq_quantize_q4_0(x, q4, M * K);
    float *w = (float *)malloc(sizeof(float) * M * K);
    gq_dequantize_q4_0(q4, w, M * nb);
    double err = 0, ref = 0;
    for (int64_t i = 0; i < M * K; ++i) {
        err += (double)(w[i] - x[i]) * (w[i] - x[i]);
        ref += (double)x[i] * x[i];
    }
    for (int64_t i = 0; i < 32; ++i)
        if (w[i] != 0.f) return printf("FAIL: the zero block gave %g\n", w[i]), 1;
    // the Q8_0 image of every block: the same d, int8 nibble - 8 in element order
    uint8_t *q8 = (uint8_t *)malloc(M * nb * 34);
    for (int64_t b = 0; b < M * nb; ++b) {
        const uint8_t *s = q4 + 18 * b;
        uint8_t *d = q8 + 34 * b;
        d[0] = s[0];
        d[1] = s[1];
        for (int i = 0; i < 16; ++i) {
            d[2 + i] = (uint8_t)(int8_t)((s[2 + i] & 15) - 8);
            d[18 + i] = (uint8_t)(int8_t)((s[2 + i] >> 4) - 8);
        }
    }
    uint16_t *a16 = (uint16_t *)malloc(sizeof(uint16_t) * N * K);
    for (int64_t i = 0; i < N * K; ++i) { // finite fp16 bits: either sign, magnitudes in [1/8, 2)
        rnd();
        a16[i] = (uint16_t)(((g_state >> 8) & 0x8000u) | 0x3000u | ((g_state >> 12) & 0x0fffu));
    }
    uint8_t *b81 = (uint8_t *)malloc(N * nb * 36);
    gq_quantize_q8_1(a16, b81, N * K);
    uint16_t *c4 = (uint16_t *)malloc(sizeof(uint16_t) * M * N), *c8 = (uint16_t *)malloc(sizeof(uint16_t) * M * N);
    for (int threads : {1, 3}) {
        if (gq_cpu_mmq(6, q4, b81, M, N, K, c4, threads) != 0) return printf("FAIL: gq_cpu_mmq type 6\n"), 1;
        if (gq_cpu_mmq(0, q8, b81, M, N, K, c8, threads) != 0) return printf("FAIL: gq_cpu_mmq type 0\n"), 1;
        if (memcmp(c4, c8, sizeof(uint16_t) * M * N) != 0) return printf("FAIL: type 6 differs from type 0 on the widened blocks\n"), 1;
    }
    if (gq_cpu_mmq(6, q4, b81, M, N, 48, c4, 1) != -1) return printf("FAIL: K = 48 accepted\n"), 1;
    printf("q4_0 host check OK: %lld blocks, round-trip relative RMSE %.4f\n", (long long)(M * nb), std::sqrt(err / ref));
    free(x), free(q4), free(w), free(q8), free(a16), free(b81), free(c4), free(c8);
    return 0;
}
