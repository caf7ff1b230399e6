// One wideband SDR recording into S receive loops (include/mercury_channelizer.h): CS16 IQ (interleaved int16 I, Q) at 48000 * D samples
// per second around a centre frequency, and a list of channel offsets from that centre. The channeliser turns the stream into one 48 kHz
// sideband audio stream per channel on the GPU and mgpu_capture_run_wideband runs the reference's receive loop (RX_SHM_process_main) on
// each of them; the audio never leaves the device. Prints every decoded payload with its channel and hop.
//
//   usage: rx_wideband <cfg> <D> <hops per call> <iq.cs16 | -> <offset_hz>[l] [<offset_hz>[l] ...] [-c carrier_hz]
//          (- reads standard input; an offset ending in l is a lower-sideband channel)
//   build: g++ -O2 -std=c++14 -I include examples/rx_wideband.cpp -L mercury_amd -lmercury_gpu -Wl,-rpath,$PWD/mercury_amd -o rx_wideband
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mercury_channelizer.h"
#include "mercury_gpu.h"

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s <cfg> <D> <hops per call> <iq.cs16 | -> <offset_hz>[l]... [-c carrier_hz]\n", argv[0]); return 2; }
    const int cfg = atoi(argv[1]), D = atoi(argv[2]), H = atoi(argv[3]);
    double carrier = 48000.0 * 50.0 / 256 / 4 / 2 + 300;                                        // physical_config.cc:84
    std::vector<mgpu_chan_channel> channels;
    for (int i = 5; i < argc; ++i) {
        if (!strcmp(argv[i], "-c") && i + 1 < argc) { carrier = atof(argv[++i]); continue; }
        const size_t n = strlen(argv[i]);
        const mgpu_chan_channel ch = {atoi(argv[i]), n && (argv[i][n - 1] == 'l' || argv[i][n - 1] == 'L') ? 1 : 0, 1.0};
        channels.push_back(ch);
    }
    const int S = int(channels.size());
    if (S < 1 || H < 1) { fprintf(stderr, "at least one channel offset and one hop per call\n"); return 2; }
    FILE* in = strcmp(argv[4], "-") ? fopen(argv[4], "rb") : stdin;
    if (!in) { perror(argv[4]); return 1; }

    mgpu_config gc = {};
    gc.cfg = cfg; gc.max_iters = 50; gc.decoder = MGPU_DEC_SPA; gc.agc = 1; gc.variance_source = 1; gc.device = 0; gc.max_batch = S;
    mgpu_ctx* rx = nullptr;
    if (mgpu_create(&gc, &rx) != MGPU_OK) { fprintf(stderr, "mgpu_create: %s\n", mgpu_last_error(nullptr)); return 1; }
    mgpu_info info;
    mgpu_get_info(rx, &info);
    const mgpu_receive_config rc = {carrier, 2, 1, 1, 0};                                      // physical_config.cc:85-87 defaults
    mgpu_capture* cap = nullptr;
    if (mgpu_capture_create(rx, S, &rc, nullptr, H, &cap) != MGPU_OK) { fprintf(stderr, "mgpu_capture_create: %s\n", mgpu_last_error(rx)); return 1; }
    mgpu_capture_geometry g;
    mgpu_capture_geometry_get(cap, &g);
    const size_t P = size_t(g.symbol_period);

    mgpu_chan_config kc = {};
    kc.struct_size = int(sizeof(kc)); kc.D = D; kc.S = S; kc.audio_centre_hz = MGPU_CHAN_DEFAULT_AUDIO_CENTRE_HZ;
    kc.taps = nullptr;                                    // the default design
    kc.max_out = int(H * P);
    mgpu_chan* chan = nullptr;
    if (mgpu_chan_create(rx, &kc, channels.data(), &chan) != MGPU_OK) { fprintf(stderr, "mgpu_chan_create: %s\n", mgpu_last_error(rx)); return 1; }
    fprintf(stderr, "%d channels at %d samples/s, %d taps, latency %d audio samples\n", S, 48000 * D, MGPU_CHAN_DEFAULT_TP * D + 1,
            mgpu_chan_latency(chan));

    const size_t n_in = H * P * size_t(D);                // IQ samples per call
    std::vector<int16_t> iq(2 * n_in);
    const int max_events = S * H;
    std::vector<mgpu_capture_event> events(max_events);
    std::vector<uint8_t> payloads(size_t(max_events) * info.payload_stride);
    long hops = 0, decoded = 0;
    while (fread(iq.data(), 2 * sizeof(int16_t), n_in, in) == n_in) {
        int n = 0;
        if (mgpu_capture_run_wideband(cap, chan, iq.data(), MGPU_IQ_CS16, H, events.data(), payloads.data(), max_events, &n) != MGPU_OK) {
            fprintf(stderr, "mgpu_capture_run_wideband: %s\n", mgpu_last_error(rx));
            return 1;
        }
        for (int e = 0; e < n && e < max_events; ++e) {
            printf("hop %ld channel %d (%+d Hz %s): SNR %5.1f dB  iterations %d  payload ", hops + events[e].hop, events[e].capture,
                   channels[events[e].capture].offset_hz, channels[events[e].capture].sideband ? "LSB" : "USB", events[e].stats.snr_db,
                   events[e].stats.iterations_done);
            for (int b = 0; b < info.payload_bytes; ++b) printf("%02x", payloads[size_t(e) * info.payload_stride + b]);
            printf("\n");
        }
        hops += H; decoded += n;
    }
    printf("%ld hops x %d channels, %ld decoded\n", hops, S, decoded);
    if (in != stdin) fclose(in);
    mgpu_chan_destroy(chan);
    mgpu_capture_destroy(cap);
    mgpu_destroy(rx);
    return 0;
}
