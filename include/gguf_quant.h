/*
 * gguf_quant.h -- C ABI of the host-side GGUF block producers (libgguf_quant.so).
 *
 * Host memory only, no GPU required.  Outputs are byte-identical to the reference's
 * producers (pinned by tests/golden/golden_quant.npz):
 *   gq_quantize_q4_k   <- utils/quantize/q4_k.py:87   quantize_to_q4_k (GGML quantize_row_q4_K_ref)
 *   gq_quantize_q6_k   <- utils/quantize/q6_k.py:97   quantize_to_q6_k (GGML quantize_row_q6_K_ref)
 *   gq_quantize_q8_0   <- utils/quantize/q8_0.py:4    quantize_to_q8_0
 *   gq_quantize_q8_1   <- utils/quantize/q8_1.py:18   quantize_to_q8_1
 *   gq_dequantize_*    <- utils/quantize/{q8_0.py:52, q8_1.py:73, q4_k.py:146, q6_k.py:138}
 *   gq_cpu_mmq         <- kernels/cpu_impls/mmq_q8_0_q8_1_cpu.py:5, mmq_q4_k_q8_1_cpu.py:61,
 *                         mmq_q6_k_q8_1_cpu.py:84 (same outputs bit for bit: fp16 running sum)
 * Beyond the reference: Q5_K (GGML type 13; the layout in include/gguf_mmq.h) --
 *   gq_quantize_q5_k   gq_quantize_q4_k's scale / min search with 31 code levels (no byte contract)
 *   gq_dequantize_q5_k (d*sc_j)*q - (dmin*m_j) in fp32, in that order
 *   gq_cpu_mmq type 3  Q4_K's terms and fp16 running sum over the 5-bit codes
 * and Q3_K (GGML type 11; the layout in include/gguf_mmq.h) --
 *   gq_quantize_q3_k   per 16 elements a scale search over codes -4..3 (gq_quantize_q6_k's), the
 *                      sixteen scales to 6 bits against the largest, codes re-fitted (no byte contract)
 *   gq_dequantize_q3_k (d*sc)*q in fp32, in that order (gq_dequantize_q6_k's)
 *   gq_cpu_mmq type 4  Q6_K's terms and fp16 running sum over codes -4..3
 * and Q2_K (GGML type 10; the layout in include/gguf_mmq.h) --
 *   gq_quantize_q2_k   per 16 elements a scale and a non-negative min over codes 0..3
 *                      (gq_quantize_q4_k's fit), the sixteen scales and mins to 4 bits against the
 *                      largest of each, codes re-fitted (no byte contract)
 *   gq_dequantize_q2_k (d*sc)*q - (dmin*m) in fp32 (both products exact: one rounding)
 *   gq_cpu_mmq type 5  per q8_1 block dB*((d*sc_lo)*i_lo + (d*sc_hi)*i_hi)
 *                      - dB*((dmin*m_lo)*sigma_lo + (dmin*m_hi)*sigma_hi), the fp16 running sum
 * and Q4_0 (GGML type 2; the layout in include/gguf_mmq.h) --
 *   gq_quantize_q4_0   per 32 elements d = m / -8 with m the element of largest magnitude, sign kept;
 *                      id = d ? 1/d : 0; code min(15, (int8)(x*id + 8.5f)); d stored as fp16.  This
 *                      is llama.cpp's rule written from memory: nothing here can check it against
 *                      llama.cpp (no byte contract).  The same code runs on the device
 *                      (gq_quantize_weights(GQ_Q4_0)), byte for byte.
 *   gq_dequantize_q4_0 d*(q - 8) in fp32 (exact)
 *   gq_cpu_mmq type 6  Q8_0's terms, in its operation order, on the codes q - 8: bit for bit
 *                      type 0 on the block's Q8_0 image
 */
#ifndef GGUF_QUANT_H
#define GGUF_QUANT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* x: n fp32 (n % 256 == 0) -> y: n/256 blocks of 144 (Q4_K) / 210 (Q6_K) bytes */
void gq_quantize_q4_k(const float *x, void *y, int64_t n);
void gq_quantize_q6_k(const float *x, void *y, int64_t n);
/* x: n fp32 (n % 256 == 0) -> y: n/256 blocks of 176 bytes (Q5_K) */
void gq_quantize_q5_k(const float *x, void *y, int64_t n);
/* x: n fp32 (n % 256 == 0) -> y: n/256 blocks of 110 bytes (Q3_K) */
void gq_quantize_q3_k(const float *x, void *y, int64_t n);
/* x: n fp32 (n % 256 == 0) -> y: n/256 blocks of 84 bytes (Q2_K) */
void gq_quantize_q2_k(const float *x, void *y, int64_t n);
/* x: n fp32 (n % 32 == 0) -> y: n/32 blocks of 18 bytes (Q4_0) */
void gq_quantize_q4_0(const float *x, void *y, int64_t n);

/* x: n fp16 bit patterns (n % 32 == 0) -> y: n/32 blocks of 34 (Q8_0) / 36 (Q8_1) bytes */
void gq_quantize_q8_0(const uint16_t *x, void *y, int64_t n);
void gq_quantize_q8_1(const uint16_t *x, void *y, int64_t n);

/* y: nblocks packed blocks -> out: nblocks * QK fp32 values in element order */
void gq_dequantize_q8_0(const void *y, float *out, int64_t nblocks);
void gq_dequantize_q8_1(const void *y, float *out, int64_t nblocks);
void gq_dequantize_q4_k(const void *y, float *out, int64_t nblocks);
void gq_dequantize_q6_k(const void *y, float *out, int64_t nblocks);
void gq_dequantize_q5_k(const void *y, float *out, int64_t nblocks);
void gq_dequantize_q3_k(const void *y, float *out, int64_t nblocks);
void gq_dequantize_q2_k(const void *y, float *out, int64_t nblocks);
void gq_dequantize_q4_0(const void *y, float *out, int64_t nblocks);

/* C (M, N) fp16 bits, row-major = the reference CPU MMQ of packed weights A (type 0 Q8_0,
 * 1 Q4_K, 2 Q6_K, 3 Q5_K, 4 Q3_K, 5 Q2_K, 6 Q4_0; M rows of K) and packed q8_1 activations B (N rows of K).  threads <= 0:
 * every hardware thread (the result does not depend on it).  0 = OK, -1 = bad type or K. */
int gq_cpu_mmq(int type, const void *A, const void *B, int64_t M, int64_t N, int64_t K, uint16_t *C, int threads);

#ifdef __cplusplus
}
#endif

#endif /* GGUF_QUANT_H */
