/* mercury_linksim.h — a link simulator: S transmitter -> HF channel -> noise -> capture-receive links on one context.
 *
 * The reference's users measure a link with two modem processes on an audio loopback, one link in real time (TX_RAND_process_main
 * sending random frames back to back, telecom_system.cc:2023-2041; RX_SHM_process_main receiving them, :2266-2390). Here every piece is
 * on the device: mgpu_transmit_byte_batch_dev makes the audio, the streaming HF channel (mercury_channel.h, mgpu_hf_stream_*) carries it
 * as one continuous signal per link, and mgpu_capture_run (mercury_capture.h) is the receive loop. Memory is bounded by one round of
 * max_hops hops, not by the run, and no sample crosses PCIe.
 *
 * Model. P = Nofdm * 4, frame_samples = mgpu_transmit_frame_samples(ctx), slot = frame_samples + gap_hops * P.
 *   - Link s sends frame j at transmit position offset_s + j * slot; offset_s in [0, slot) is a Philox draw keyed by (seed, s), so links
 *     are aligned neither to hops nor to each other. Between its frames a transmitter is silent (zeros). The payload of (s, j) is
 *     payload_bytes Philox bytes keyed by (seed, s, j); the audio is mgpu_transmit_byte_batch_dev's (SINGLE_MESSAGE, every frame from
 *     tx.start_sample).
 *   - The transmit stream goes through the streaming channel at 48 kHz (realisation = link index, latency L = 256 samples) with
 *     noise_amp[s] derived from esn0_db[s] as mgpu_passband_test_esn0 derives it: OFDM 1 / sqrt(10^(EsN0/10)) / sqrt(2); MFSK calibrated
 *     from the mean power of the first frame link 0 sends.
 *   - The channel's output is what mgpu_capture_run is given (MGPU_SAMPLES_F64, device memory). The capture starts from zero windows.
 *   - Bookkeeping on the host, per decoded event of link s at hop h (a decode happens after hop h's samples, so (h + 1) * P samples have
 *     been received): frame j is matchable when its last sample e_j = offset_s + j * slot + frame_samples - 1 + L has been received and
 *     lies less than one capture window in the past (e_j <= (h + 1) P - 1 < e_j + window). A payload equal to a matchable frame not yet
 *     delivered: `delivered`; equal to a matchable frame already delivered: `duplicates`; crc good and equal to neither: `false_decodes`.
 *     frames_sent counts frames whose last sample has been fed to the channel.
 */
#ifndef MERCURY_LINKSIM_H
#define MERCURY_LINKSIM_H

#include <stdint.h>

#include "mercury_capture.h"
#include "mercury_channel.h"
#include "mercury_gpu.h"
#include "mercury_rxloop.h"
#include "mercury_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgpu_linksim mgpu_linksim;

typedef struct mgpu_linksim_config {
    int struct_size;                 /* = sizeof(mgpu_linksim_config), else MGPU_ERR_ARG (versioned by size, as mgpu_hf_channel) */
    int S;                           /* links, >= 1 */
    int gap_hops;                    /* silence between a link's frames in hops, >= 0 (0: back to back, as TX_RAND_process_main sends) */
    int max_hops;                    /* hops per internal round (0: 16); also the capture's max_hops */
    uint64_t seed;
    mgpu_hf_channel channel;         /* identity allowed */
    mgpu_receive_config rx;
    mgpu_transmit_config tx;         /* MGPU_SINGLE_MESSAGE only; every link is its own transmitter */
} mgpu_linksim_config;

typedef struct mgpu_linksim_counters {        /* per link, since create */
    long long hops, frames_sent, delivered, duplicates, false_decodes;
    long long iterations_sum;                  /* over delivered frames: all of this comes from mgpu_capture_run's events, */
    double snr_db_sum;                         /* which report decoded frames only                                         */
} mgpu_linksim_counters;

/* esn0_db: [S] host doubles, NULL: no noise */
int mgpu_linksim_create(mgpu_ctx* ctx, const mgpu_linksim_config* config, const double* esn0_db, mgpu_linksim** out);
int mgpu_linksim_destroy(mgpu_linksim* sim);
/* H more hops for every link. events / payloads / max_events / n_events as mgpu_capture_run, hop counted from the simulator's start.
 * samples_out: NULL or [S][H * P] host doubles, the audio the captures were fed (for tests). */
int mgpu_linksim_run(mgpu_linksim* sim, int H, mgpu_capture_event* events, uint8_t* payloads, int max_events, int* n_events, double* samples_out);
int mgpu_linksim_counters_get(mgpu_linksim* sim, mgpu_linksim_counters* out /* [S] */);
/* the capture inside (mgpu_capture_get_state, mgpu_capture_window); it belongs to the simulator */
int mgpu_linksim_capture(mgpu_linksim* sim, mgpu_capture** cap);
/* the noise amplitude per link that esn0_db gave ([S]; zeros without noise): the streaming channel's noise_amp */
int mgpu_linksim_noise_amp(mgpu_linksim* sim, double* out);

/* host only: the schedule and the payloads, so a caller can rebuild what was sent. frame_samples and symbol_period are the context's
 * (mgpu_transmit_frame_samples, Nofdm * 4); of `config` the fields struct_size, S, gap_hops, seed and tx.message_location are read. */
int mgpu_host_linksim_frame_start(const mgpu_linksim_config* config, int frame_samples, int symbol_period, int link, long long frame,
                                  long long* start_sample);
int mgpu_host_linksim_payload(uint64_t seed, int link, long long frame, int nbytes, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MERCURY_LINKSIM_H */
