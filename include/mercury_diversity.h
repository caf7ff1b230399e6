/* mercury_diversity.h — diversity combining: D copies (branches) of one transmitted frame decoded from the sum of their LLRs.
 *
 * A second receiver or antenna, or a retransmission, gives a second copy of a frame. Each copy goes through the front-end on its own
 * (its own synchronisation, channel estimate, equalisation and noise variance); the decoder then runs once per transmitted frame, on the
 * sum of the copies' LLRs. This is NOT one of the reference's configurations: the reference decodes every frame alone.
 *
 * The rule. A batch of F = G * D frames holds G groups; frames g*D .. g*D+D-1 are the D branches of group g, D = 1..MGPU_DIVERSITY_MAX.
 * The combined LLR vector of a group is
 *     out[g][i] = (..((llr[m0][i] + llr[m1][i]) + llr[m2][i]) ..),   i < 1600,
 * float additions in member order: no reassociation, no weights, +-Inf and NaN as IEEE addition gives them; a group of one is a copy.
 * The decoder (the context's, unchanged) runs on the G combined rows, and every member row f of group g then reports
 *     payload[f]                                                  = the group's payload
 *     stats[f].iterations_done, crc, all_zeros, message_decoded   = the group's
 *     stats[f].variance                                           = branch f's own
 *     stats[f].snr_db                                             = branch f's own SNR where the group decoded, -99.9 where it did not
 * so each row reads as if the decoder had written it for that frame (in the zero-forcing modes snr_db is the error vector of branch f's
 * own equalised symbols against the group's re-encoded payload). D = 1 gives, byte for byte, what mgpu_rx_batch_dev gives.
 *
 * What the sum is. The front-end's LLRs are already scaled by 1 / variance. In the PSK modes (amp_restore: CONFIG_0..14) the equalised
 * cell keeps |H|, so for BPSK and QPSK the sum of two branches' LLRs is maximal-ratio combining, and for 8PSK it is close to it (the
 * max-log demapper is not linear in the cell). In the QAM and zero-forcing modes (the cell is divided by H) and in the MFSK modes it is
 * plain post-detection combining of per-branch soft decisions: still a gain, not the optimum. With the channel-aware demapper
 * (mercury_demapper.h: MGPU_DEMAP_CSI on the context) every branch's LLRs carry |H|^2 / sigma2 per cell, and the sum is maximal-ratio
 * combining for every constellation.
 *
 * Out of scope here, each untouched by this header:
 *   - mgpu_receive_byte_batch, mgpu_capture_*, mgpu_linksim_* and the passband self-simulations do not combine: the synchroniser, not
 *     the decoder, sets their AWGN floor, so combining there needs a design of its own (joint synchronisation of the branches);
 *   - mgpu_pool_* does not forward these entry points; call them on each mgpu_pool_context;
 *   - estimator ladders with retries (more than one rung) are refused with MGPU_ERR_UNSUPPORTED: a retry would have to re-estimate whole
 *     groups. A one-rung ladder is accepted: its window is the front-end's and nothing is retried (its rung marks and counters are not
 *     updated by a grouped call);
 *   - a pipelined host path: mgpu_rx_batch_div is one upload, one run, one download.
 *
 * Refused with MGPU_ERR_ARG before any device work, outputs untouched: D outside 1..MGPU_DIVERSITY_MAX, F % D != 0, F > max_batch, a
 * CSR whose `first` does not start at 0 or decreases, a CSR group that is empty or has more than MGPU_DIVERSITY_MAX members, a CSR member
 * outside [0, F).
 */
#ifndef MERCURY_DIVERSITY_H
#define MERCURY_DIVERSITY_H

#include <stdint.h>

#include "mercury_channel.h"
#include "mercury_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_DIVERSITY_MAX 8

/* The fused receive span on F = G * D frames in device memory, enqueued on `stream`: front-end on every frame, combine, decoder on the G
 * sums, results to all F rows as described above. d_llr_opt, when given, receives the BRANCH LLRs ([F][1600], what mgpu_rx_batch_dev
 * writes there), not the sums: they are what a caller keeps for combining with a later copy. */
int mgpu_rx_batch_div_dev(mgpu_ctx* ctx, const void* d_baseband, int F, int D, void* d_payload /*[F][payload_stride]*/,
                          void* d_stats /*[F]*/, void* d_llr_opt /*[F][1600] or NULL*/, void* stream);

/* The same on host buffers, blocking: one upload, one run, one download (no chunked pipeline). payload, stats, llr_opt may be NULL. */
int mgpu_rx_batch_div(mgpu_ctx* ctx, const double* baseband, int F, int D, uint8_t* payload, mgpu_frame_stats* stats, float* llr_opt);

/* The combining step alone, on F rows of LLRs in device memory, enqueued on `stream`. first == NULL and member == NULL: uniform groups
 * of D (F % D == 0, G is ignored: F / D rows are written). Otherwise a CSR in HOST memory, and D is ignored: group g sums the rows
 * member[first[g]] .. member[first[g+1]-1] in that order, first[0] == 0, 1..MGPU_DIVERSITY_MAX members per group, each in [0, F); a row
 * may belong to any number of groups. d_out: [G][1600], not overlapping d_llr. Rows are moved as 16-byte vectors when d_llr and d_out
 * are 16-byte aligned, one float at a time otherwise; the sums are the same. */
int mgpu_llr_combine_dev(mgpu_ctx* ctx, const void* d_llr, int F, int D, const int* first /*[G+1]*/, const int* member, int G,
                         void* d_out, void* stream);

/* Host twin, no GPU and no context: the same additions in the same order on host arrays. F bounds the member rows only. */
int mgpu_host_llr_combine(const float* llr /*[F][1600]*/, int F, int D, const int* first, const int* member, int G, float* out);

/* mgpu_baseband_test_esn0_hf (mercury_channel.h) with D branches per payload. groups_per_point counts payloads: per point, group number
 * q = frame0 + point * groups_per_point + k keys the payload and the clean frame (what frame number q keys in the plain loop), and branch d
 * of it is channel realisation and noise of frame number q * D + d - whatever the batch size. The decoder runs once per group and the
 * counters count groups: Frames_total == groups_per_point. ch: the identity preset (MGPU_HF_AWGN) for AWGN. With D = 1 every record
 * equals mgpu_baseband_test_esn0_hf's. D > max_batch is refused (a group does not fit one launch). */
int mgpu_baseband_test_esn0_div(mgpu_ctx* ctx, const double* esn0_db, int npoints, long long groups_per_point, uint64_t seed, uint64_t frame0,
                                const mgpu_hf_channel* ch, int D, mgpu_error_rate* out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_DIVERSITY_H */
