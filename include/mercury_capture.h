/* mercury_capture.h — the reference's receive loop over continuous captures (RX_SHM_process_main with its capture-prep thread), batched.
 *
 * The reference's production receiver is a loop over one continuous audio capture, split across two threads:
 *
 *   capture prep (radio_capture_prep_thread, audioio.c:999-1069): for every symbol period P = Nofdm * 4 of new audio it slides the
 *   window passband_delayed_data left by P (shift_left, misc.cc:26-32), writes the new samples at sp - P - 1 (:1035, :1050-1051), counts
 *   frames_to_read down to 0 (:1053-1055) and nUnder_processing_events up when the previous window was not processed yet (:1047-1048);
 *
 *   process (RX_SHM_process_main, telecom_system.cc:2266-2390; RX_RAND_process_main :2146-2170 keeps the same bookkeeping): receive_byte
 *   on the window when frames_to_read == 0; after a decode frames_to_read skips the rest of the frame, delay_of_last_decoded_message
 *   moves forward and nUnder is reset; without one delay_of_last_decoded_message moves back by one symbol (:2304-2377).
 *
 * An mgpu_capture holds S such captures on one context (one configuration, one mgpu_receive_config). Each capture's window lives on the
 * device as a ring of its last sp - 1 samples plus the one sample the loop never overwrites (sp = buffer_Nsymb * P); a feed uploads only
 * the new hops, and the windows that receive_byte reads are gathered from the rings into one device array per hop. Per capture:
 *
 *   feed, per hop:  if (data_ready) nUnder++;  window[j] = window[j + P] for j < sp - P;  window[sp-P-1 .. sp-2] = widen(next P samples);
 *                   frames_to_read = max(0, frames_to_read - 1);  data_ready = 1          (window[sp-1] keeps its initial value forever)
 *   process:        if (data_ready && frames_to_read == 0): receive_byte with MFSK search start max(0, mfsk_search_raw - nUnder), then
 *                   on a decode: frames_left = max(0, buffer_Nsymb - (delay / P + Nsymb + pre));
 *                                frames_to_read = Nsymb + pre - frames_left - nUnder, or Nsymb + pre - frames_left when that is outside
 *                                [0, Nsymb + pre];  delay_of_last_decoded_message += (Nsymb + pre - frames_to_read) * P;  nUnder = 0
 *                   otherwise:   delay_of_last_decoded_message -= P unless it is -1; below 0 it becomes -1
 *                   data_ready = 0
 *
 * Nsymb is data_container.Nsymb, the configuration's, also in MFSK control mode (the reference's loop does not use get_active_nsymb).
 * Widening is the capture thread's (audioio.c:893-936): INT32 x / 2147483647.0, INT16 x / 32768.0, FLOAT32 widened, F64 as is.
 * Every call feeds all S captures the same number of hops (radios on one sound clock). run(H) is H rounds of feed(1) + process(): the
 * reference when its process thread keeps up; feed(k) + process() is the reference when it falls k - 1 hops behind.
 *
 * Errors as mercury_gpu.h (MGPU_ERR_ARG for bad sizes, formats or null pointers); the context rules of INTEGRATION.md §2 apply: an
 * mgpu_capture belongs to its context, is used by one thread at a time with it and is destroyed before it.
 */
#ifndef MERCURY_CAPTURE_H
#define MERCURY_CAPTURE_H

#include <stdint.h>

#include "mercury_gpu.h"
#include "mercury_rxloop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgpu_capture mgpu_capture;

/* st_receive_stats as the reference's member holds it between receive_byte calls (telecom_system.h:63-82; the stale-field rules of
 * INTEGRATION.md §1.3b). Starts as the constructor leaves it (telecom_system.cc:38-51): iterations_done -1, SNR -99.9,
 * signal_strength_dbm -999, the rest 0. */
typedef struct mgpu_capture_held_stats {
    int iterations_done, message_decoded, crc, all_zeros, delay, sync_trials, frame_overflow_symbols;
    double snr_db, freq_offset, coarse_metric, signal_strength_dbm;
} mgpu_capture_held_stats;

/* one capture's loop state: data_container.frames_to_read / nUnder_processing_events / data_ready, receive_stats.mfsk_search_raw (the
 * ARQ layer sets it), the cross-call link state (link.mfsk_search_start is derived for each call and not kept) and the held stats */
typedef struct mgpu_capture_state {
    int frames_to_read;             /* starts at preamble_nSymb + Nsymb (data_container.cc:155); a decode near the window's start leaves it
                                       negative, as in the reference, and the next hop's capture prep clamps it to 0 */
    int n_under;                    /* nUnder_processing_events, starts at 0 */
    int data_ready;                 /* starts at 0 */
    int mfsk_search_raw;            /* starts at 0 */
    mgpu_link_state link;           /* starts with delay_of_last_decoded_message = -1 */
    mgpu_capture_held_stats held;
} mgpu_capture_state;

/* the loop's sizes, as the host twins take them */
typedef struct mgpu_capture_geometry {
    int buffer_nsymb, nsymb, preamble_nsymb, symbol_period;   /* symbol_period P = Nofdm * 4; a window is buffer_nsymb * P samples */
    int mfsk;                                                 /* 1 in the MFSK modes (which fields receive_byte writes) */
} mgpu_capture_geometry;

/* a decoded frame of mgpu_capture_run: capture index, hop of the call (0-based) after which it was decoded, receive_byte's statistics */
typedef struct mgpu_capture_event {
    int capture, hop;
    mgpu_receive_stats stats;
} mgpu_capture_event;

/* S captures on ctx. initial_windows: NULL (zeros) or [S][sp] doubles in host memory (the reference fills its window with
 * (rand() % 1000 - 500) / 1000.0, data_container.cc:168-171). max_hops: hops one feed uploads at once (0: 16); longer calls are split.
 * The state of every capture starts as mgpu_capture_state describes. */
int mgpu_capture_create(mgpu_ctx* ctx, int S, const mgpu_receive_config* config, const double* initial_windows, int max_hops, mgpu_capture** out);
int mgpu_capture_destroy(mgpu_capture* cap);
int mgpu_capture_geometry_get(mgpu_capture* cap, mgpu_capture_geometry* g);

/* H hops of capture prep for every capture. samples: [S][H * P] in sample_format (MGPU_SAMPLES_*), host or device memory (detected). */
int mgpu_capture_feed(mgpu_capture* cap, const void* samples, int sample_format, int H);

/* One process step for every capture. ran: [S] (1 = receive_byte ran on the capture's window). stats: [S], payload: [S][payload_stride]
 * (mgpu_get_info), written where ran is 1 and left alone elsewhere; any of the three may be NULL. Host arrays. */
int mgpu_capture_process(mgpu_capture* cap, int* ran, mgpu_receive_stats* stats, uint8_t* payload);

/* H rounds of feed(1) + process() with the samples uploaded in one copy (per max_hops). The decoded frames in order of hop, then capture:
 * events [max_events] and payloads [max_events][payload_stride] (host, either may be NULL when max_events is 0). *n_events: how many there
 * were; only the first max_events are written (at most S * H can occur). */
int mgpu_capture_run(mgpu_capture* cap, const void* samples, int sample_format, int H, mgpu_capture_event* events, uint8_t* payloads,
                     int max_events, int* n_events);

/* one capture's loop state (checkpoints, tests, callers that set mfsk_search_raw) */
int mgpu_capture_get_state(mgpu_capture* cap, int s, mgpu_capture_state* st);
int mgpu_capture_set_state(mgpu_capture* cap, int s, const mgpu_capture_state* st);
/* a copy of capture s's current window, [sp] doubles into host memory */
int mgpu_capture_window(mgpu_capture* cap, int s, double* window);

/* Host-only twins (no GPU), the code the device path runs for its bookkeeping:
 * mgpu_host_capture_prep: one hop of capture prep (audioio.c:1035-1057) on a host window of g->buffer_nsymb * P doubles, samples [P] in
 * sample_format. mgpu_host_capture_process: the process step around one receive_byte result (telecom_system.cc:2304-2377): when
 * st->data_ready and st->frames_to_read == 0, r is receive_byte's result on the window and link its link state afterwards (as
 * mgpu_receive_byte_batch leaves it); otherwise neither is read. Returns 1 when the step is one that ran receive_byte, 0 when not, < 0 on
 * an error (-MGPU_ERR_ARG). mgpu_host_capture_init_state: the state a capture starts with. */
int mgpu_host_capture_prep(const mgpu_capture_geometry* g, double* window, const void* samples, int sample_format, mgpu_capture_state* st);
int mgpu_host_capture_process(const mgpu_capture_geometry* g, mgpu_capture_state* st, const mgpu_receive_stats* r, const mgpu_link_state* link);
int mgpu_host_capture_init_state(const mgpu_capture_geometry* g, mgpu_capture_state* st);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_CAPTURE_H */
