// RX_SHM_process_main over S continuous recordings (include/mercury_capture.h): the reference's capture-prep thread
// (audioio.c:999-1069) and process loop (telecom_system.cc:2266-2390) for S captures at once, every capture's window kept on the GPU.
// Each step reads one symbol period (Nofdm * 4 samples) per capture, runs one round of feed + process (mgpu_capture_run with H = 1)
// and publishes the decoded payloads to the "/mercury-comm" ring that client programs read (examples/receiver.c), as rx_shm_batch.cpp does.
//
// Recordings are raw samples: .f64 (doubles), .i32 (what the reference's capture thread asks for, audioio.c:744), .i16 or .f32. Either one
// file per capture, or with S > 1 and a single file, S captures interleaved sample by sample (one multi-channel recording).
//
//   usage: rx_capture <cfg> <S> <hops per call> <recording> [<recording> ...] [-c carrier_hz]
//   build: g++ -O2 -std=c++14 -I include examples/rx_capture.cpp -L mercury_amd -lmercury_gpu -Wl,-rpath,$PWD/mercury_amd -o rx_capture
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mercury_capture.h"
#include "mercury_gpu.h"
#include "mercury_rxloop.h"
#include "mercury_shm.h"

static int format_of(const char* path) {
    const char* ext = strrchr(path, '.');
    return ext && !strcmp(ext, ".i32") ? MGPU_SAMPLES_INT32 : ext && !strcmp(ext, ".i16") ? MGPU_SAMPLES_INT16 :
           ext && !strcmp(ext, ".f32") ? MGPU_SAMPLES_F32 : MGPU_SAMPLES_F64;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s <cfg> <S> <hops per call> <recording>... [-c carrier_hz]\n", argv[0]); return 2; }
    const int cfg = atoi(argv[1]), S = atoi(argv[2]), H = atoi(argv[3]);
    double carrier = 48000.0 * 50.0 / 256 / 4 / 2 + 300;                                        // physical_config.cc:84
    std::vector<const char*> files;
    for (int i = 4; i < argc; ++i) {
        if (!strcmp(argv[i], "-c") && i + 1 < argc) carrier = atof(argv[++i]);
        else files.push_back(argv[i]);
    }
    if (S < 1 || H < 1 || (files.size() != 1 && int(files.size()) != S)) { fprintf(stderr, "one recording per capture, or one interleaved\n"); return 2; }
    const bool interleaved = files.size() == 1 && S > 1;
    const int fmt = format_of(files[0]);
    const size_t sample = fmt == MGPU_SAMPLES_F64 ? 8 : fmt == MGPU_SAMPLES_INT16 ? 2 : 4;

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

    mgpu_shm* ring = nullptr;
    if (mgpu_shm_connect(MGPU_SHM_PAYLOAD_NAME, MGPU_SHM_PAYLOAD_BUFFER_SIZE, &ring) != MGPU_OK &&
        mgpu_shm_create(MGPU_SHM_PAYLOAD_NAME, MGPU_SHM_PAYLOAD_BUFFER_SIZE, &ring) != MGPU_OK) { fprintf(stderr, "cannot open the payload ring\n"); return 1; }

    std::vector<FILE*> in;
    for (const char* p : files) {
        FILE* f = fopen(p, "rb");
        if (!f) { perror(p); return 1; }
        in.push_back(f);
    }
    const size_t row = H * P * sample;                    // one capture's samples of one call
    std::vector<char> samples(S * row), inter(interleaved ? S * row : 0);
    const int max_events = S * H;
    std::vector<mgpu_capture_event> events(max_events);
    std::vector<uint8_t> payloads(size_t(max_events) * info.payload_stride);
    std::vector<mgpu_frame_stats> fstats(max_events);
    long hops = 0, decoded = 0, lost = 0;
    for (;;) {
        bool eof = false;
        if (interleaved) {                                // [H*P][S] -> [S][H*P]
            eof = fread(inter.data(), S * sample, H * P, in[0]) != H * P;
            for (size_t i = 0; i < H * P && !eof; ++i)
                for (int s = 0; s < S; ++s) memcpy(&samples[s * row + i * sample], &inter[(i * S + s) * sample], sample);
        } else {
            for (int s = 0; s < S && !eof; ++s) eof = fread(&samples[s * row], 1, row, in[s]) != row;
        }
        if (eof) break;                                   // every capture advances by the same hops: stop at the shortest recording
        int n = 0;
        if (mgpu_capture_run(cap, samples.data(), fmt, H, events.data(), payloads.data(), max_events, &n) != MGPU_OK) {
            fprintf(stderr, "mgpu_capture_run: %s\n", mgpu_last_error(rx));
            return 1;
        }
        for (int e = 0; e < n; ++e) { fstats[e] = mgpu_frame_stats(); fstats[e].message_decoded = 1; }
        int pub = 0, drop = 0;
        mgpu_shm_publish_decoded(ring, payloads.data(), fstats.data(), n, info.payload_stride, info.payload_bytes, &pub, &drop);   // :2323-2336
        for (int e = 0; e < n; ++e)
            printf("hop %ld capture %d: decoded  SNR %5.1f dB  level %6.1f dBm  delay %d  iterations %d\n", hops + events[e].hop,
                   events[e].capture, events[e].stats.snr_db, events[e].stats.signal_strength_dbm, events[e].stats.delay,
                   events[e].stats.iterations_done);
        hops += H; decoded += n; lost += drop;
    }
    printf("%ld hops x %d captures, %ld decoded, %ld lost to a full ring\n", hops, S, decoded, lost);
    for (FILE* f : in) fclose(f);
    mgpu_shm_close(ring);
    mgpu_capture_destroy(cap);
    mgpu_destroy(rx);
    return 0;
}
