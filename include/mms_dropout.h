/* include/mms_dropout.h -- Dropout on the C ABI of libmms_hip.so: the reference's DropoutLayer arithmetic
 * (dropout_layer.cpp:14-18, 31-65; dropout_layer.cu:13, 42) over a mask that a counter-based generator defines, so that
 * the backward regenerates the mask and no rand_vec_ is stored.  network_v4 has two: Dropout(0.1) on the SimCross top
 * (do_trec_qa_clean.py:470) and Dropout(0.5) inside the classifier head (:485), whose mask mms_dropout_mask_u32 draws in
 * the format include/mms_head.h takes.
 *
 * This header adds to include/mms.h and changes nothing in it: the error codes, the stream convention (`stream` is a
 * hipStream_t, NULL = the default stream) and MMS_VERSION are those of mms.h.  All arrays are device memory and
 * contiguous; a call enqueues one launch on `stream` and returns without waiting; it allocates nothing, synchronises
 * nothing and uses no atomics.  Dtype is float (_f32) or double (_f64).
 *
 * The random words.  The reference draws its mask with cuRAND's default generator (GPU) or boost's Bernoulli (CPU);
 * neither is reproduced.  Here the word of an element is a pure function of (seed, sequence, g), g the element's GLOBAL
 * index: g = offset + i (64-bit), i the index within the call.
 *
 *   ctr = (lo32(g >> 2), hi32(g >> 2), lo32(sequence), hi32(sequence))       key = (lo32(seed), hi32(seed))
 *   word(g) = Philox4x32-10(ctr, key)[g & 3]
 *
 * Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123), ten
 * rounds; one round maps (c0, c1, c2, c3) under key (k0, k1) to
 *
 *   (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))     M0 = 0xD2511F53, M1 = 0xCD9E8D57
 *
 * hi / lo the halves of the 64-bit product, and between two rounds the key is bumped by (0x9E3779B9, 0xBB67AE85),
 * modulo 2^32.  Known answers (Random123's):
 *
 *   ctr 00000000 00000000 00000000 00000000  key 00000000 00000000  ->  6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   ctr ffffffff ffffffff ffffffff ffffffff  key ffffffff ffffffff  ->  408f276d 41c83b0e a20bc7c6 6d5451fd
 *   ctr 243f6a88 85a308d3 13198a2e 03707344  key a4093822 299f31d0  ->  d16cfe09 94fdcceb 5001e420 24126ea1
 *
 * So a result depends on no launch geometry and on no alignment of the arrays, and a blob cut into pieces (a batch
 * sharded over devices) gives the words of the whole when piece k passes offset = the number of elements before it.
 * The HOST chooses `sequence`: one value per (layer, iteration), the same in that iteration's forward and backward.
 * Reusing a (seed, sequence) pair repeats the mask: two layers, or two iterations, that share one drop the same
 * elements.  The library keeps no counter.
 *
 * Keep rule and arithmetic, the reference's; r = Dtype(ratio):
 *
 *   thr   = (unsigned)(Dtype(UINT_MAX) * r)      one product in Dtype; Dtype(UINT_MAX) is 2^32 in float     .cpp:18
 *   scale = Dtype(1. / (1. - r))                 in double, then narrowed                                   .cpp:17
 *   keep  = word > thr                                                                                     .cu:13
 *   y  = (x  * Dtype(keep)) * scale              two roundings.  A dropped -x gives -0, a dropped Inf or   .cpp:41
 *   dx = (dy * Dtype(keep)) * scale              NaN gives NaN, as in the reference.                       .cpp:59
 *   TEST: y = x (dx = dy), a copy; nothing at all when in place                                            .cpp:44, 62
 *   Every word of y is pinned by this but the sign and payload of a NaN result, which are the multiplier's.
 *
 * mms_dropout_mask_u32 writes Dtype-free words, keep as 0 or 1: the format of the reference's CPU rand_vec_, and what
 * mms_head_forward_* / mms_head_backward_* take as `mask`.  Its _f64 twin differs in thr alone (computed in double).
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   MMS_ERR_INVALID_ARG  ratio not in (0, 1) (0, 1, negatives and NaN among them), in TEST too; a ratio for which
 *                        Dtype(UINT_MAX) * r does not fit 32 bits (the reference's cast is undefined there); a NULL
 *                        thr or scale (threshold calls); a phase that is neither MMS_DROPOUT_TRAIN nor _TEST;
 *                        count < 0 or > INT_MAX (Caffe's count()); offset + count wrapping 2^64; with count > 0: a
 *                        NULL array, or x and y (dy and dx) overlapping other than y == x, which is the in-place form.
 *   count == 0           MMS_OK, nothing is written, the pointers are not looked at.
 */
#ifndef MMS_DROPOUT_H_
#define MMS_DROPOUT_H_

#include "mms.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_DROPOUT_TRAIN 0               /* caffe.proto: Phase */
#define MMS_DROPOUT_TEST 1

/* The launch plan, stated because a test has to step past it: a lane owns whole Philox groups (four consecutive global
 * indices, the first a multiple of 4), a workgroup has MMS_DROPOUT_THREADS lanes, a launch at most
 * MMS_DROPOUT_MAX_BLOCKS workgroups, and a lane of forward / backward takes MMS_DROPOUT_GROUPS_PER_TRIP groups per trip
 * of its loop (the mask writer one), so one trip of the largest grid covers THREADS * MAX_BLOCKS * GROUPS_PER_TRIP * 4
 * elements; the lanes stride over the groups beyond that.  No result depends on it. */
#define MMS_DROPOUT_THREADS 256
#define MMS_DROPOUT_MAX_BLOCKS 2048
#define MMS_DROPOUT_GROUPS_PER_TRIP 2

/* thr and scale as the calls below compute them from ratio.  Host only: nothing is enqueued. */
int mms_dropout_threshold_f32(float ratio, unsigned int* thr, float* scale);
int mms_dropout_threshold_f64(double ratio, unsigned int* thr, double* scale);

int mms_dropout_forward_f32(const float* x, float* y, long long count, float ratio, int phase,
                            unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                            void* stream);
int mms_dropout_forward_f64(const double* x, double* y, long long count, double ratio, int phase,
                            unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                            void* stream);
/* The same map on the diffs, with the forward's (ratio, phase, seed, sequence, offset): the mask is regenerated. */
int mms_dropout_backward_f32(const float* dy, float* dx, long long count, float ratio, int phase,
                             unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                             void* stream);
int mms_dropout_backward_f64(const double* dy, double* dx, long long count, double ratio, int phase,
                             unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                             void* stream);

/* mask[i] = word(offset + i) > thr ? 1 : 0.  _u32: thr as the _f32 calls have it; _u32_f64: as the _f64 calls. */
int mms_dropout_mask_u32(unsigned int* mask, long long count, float ratio, unsigned long long seed,
                         unsigned long long sequence, unsigned long long offset, void* stream);
int mms_dropout_mask_u32_f64(unsigned int* mask, long long count, double ratio, unsigned long long seed,
                             unsigned long long sequence, unsigned long long offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_DROPOUT_H_ */
