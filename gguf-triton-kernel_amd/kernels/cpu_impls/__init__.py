"""Drop-in for the reference's `kernels.cpu_impls` package: the CPU MMQ products with the
reference's exact arithmetic (fp16 running sum in block order), run by libgguf_quant.so
(csrc/quant/gguf_cpu_mmq.cpp, multithreaded C++).  Host tensors only; the GPU entry points
in `kernels.mmq_*` never call these.  mmq_q5_k_q8_1_cpu (Q5_K),
mmq_q3_k_q8_1_cpu (Q3_K), mmq_q2_k_q8_1_cpu (Q2_K) and mmq_q4_0_q8_1_cpu (Q4_0) have no reference
counterpart."""
