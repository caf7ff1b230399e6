"""The C ABI of ``libmercury_gpu.so`` as Python states it: one prototype per ``mgpu_*`` function, grouped by the header under
``include/`` (``PROTOTYPES``) or ``include/ext/`` (``EXTENSIONS``) that declares it, and ``load_library()``, which applies all of them once.

A signature is ``"<return>:<one letter per parameter>"``:

    i int     z size_t     u uint64_t     q long long     d double     s const char*
    p any other pointer or array parameter (mgpu_ctx**, double out[4], a writable char*)
    returns also: v void, l long, p void* or mgpu_ctx*

The table is written by hand. tests/test_abi.py parses the headers and compares, in both directions: the two statements are
independent on purpose.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MERCURY_GPU_LIB: another build of the same HIP library (kernel experiments: tools/build_variants.sh); never a CPU path
LIB_PATH = os.environ.get("MERCURY_GPU_LIB") or os.path.join(HERE, "libmercury_gpu.so")

PROTOTYPES = {
    "mercury_blanker.h": {
        "mgpu_set_blanker": "i:pipz", "mgpu_get_blanker": "i:pppz", "mgpu_get_blanker_report": "i:piip", "mgpu_blank_dev": "i:ppiippp",
        "mgpu_host_blank": "i:ippppp",
    },
    "mercury_capture.h": {
        "mgpu_capture_create": "i:pippip", "mgpu_capture_destroy": "i:p", "mgpu_capture_geometry_get": "i:pp", "mgpu_capture_feed": "i:ppii",
        "mgpu_capture_process": "i:pppp", "mgpu_capture_run": "i:ppiippip", "mgpu_capture_get_state": "i:pip", "mgpu_capture_set_state": "i:pip",
        "mgpu_capture_window": "i:pip", "mgpu_host_capture_prep": "i:pppip", "mgpu_host_capture_process": "i:pppp",
        "mgpu_host_capture_init_state": "i:pp",
    },
    "mercury_cfo.h": {
        "mgpu_set_cfo": "i:pi", "mgpu_get_cfo": "i:pp", "mgpu_get_cfo_steps": "i:pip", "mgpu_host_cfo_pilots": "i:ipppp",
    },
    "mercury_channel.h": {
        "mgpu_hf_channel_preset": "i:ip", "mgpu_host_hilbert_taps": "i:pp", "mgpu_host_hf_channel_draws": "i:puuipp",
        "mgpu_host_hf_channel_taps": "i:pduuqip", "mgpu_hf_channel_apply": "i:pppidiiuuqp", "mgpu_hf_channel_apply_dev": "i:pppidiiuuqpp",
        "mgpu_hf_stream_create": "i:ppdiuup", "mgpu_hf_stream_destroy": "i:p", "mgpu_hf_stream_seek": "i:pu", "mgpu_hf_stream_latency": "i:p",
        "mgpu_hf_stream_apply": "i:ppipp", "mgpu_hf_stream_apply_dev": "i:ppippp", "mgpu_host_hf_stream_noise": "i:uiuip",
        "mgpu_passband_test_esn0_hf": "i:ppiquuddpppp", "mgpu_baseband_test_esn0_hf": "i:ppiquupp",
    },
    "mercury_channelizer.h": {
        "mgpu_chan_create": "i:pppp", "mgpu_chan_destroy": "i:p", "mgpu_chan_latency": "i:p", "mgpu_chan_seek": "i:pu", "mgpu_chan_retune": "i:pip",
        "mgpu_chan_process": "i:ppiip", "mgpu_chan_process_dev": "i:ppiipp", "mgpu_capture_run_wideband": "i:pppiippip",
        "mgpu_host_chan_design": "i:iiddpp", "mgpu_host_chan_default_taps": "i:ipp", "mgpu_host_chan_tables": "i:pppp",
        "mgpu_host_chan_process": "i:pppiiup",
    },
    "mercury_demapper.h": {
        "mgpu_set_demapper": "i:pi", "mgpu_get_demapper": "i:pp", "mgpu_set_demapper_ex": "i:pipz", "mgpu_get_demapper_ex": "i:pppz",
        "mgpu_get_noise_map": "i:piipp", "mgpu_host_demap_csi": "i:ippppp", "mgpu_host_demap_nmap": "i:ippppzpppp",
    },
    "mercury_diversity.h": {
        "mgpu_rx_batch_div_dev": "i:ppiipppp", "mgpu_rx_batch_div": "i:ppiippp", "mgpu_llr_combine_dev": "i:ppiippipp",
        "mgpu_host_llr_combine": "i:piippip", "mgpu_baseband_test_esn0_div": "i:ppiquupip",
    },
    "mercury_estimator.h": {
        "mgpu_set_estimator_ladder": "i:ppi", "mgpu_get_estimator_ladder": "i:ppp", "mgpu_set_estimator_ladder_ex": "i:ppiz",
        "mgpu_get_estimator_ladder_ex": "i:pppz", "mgpu_estimator_rungs_last": "i:ppi", "mgpu_estimator_ladder_counters": "i:pppi",
        "mgpu_host_ls_estimate": "i:ipiipp", "mgpu_host_wiener_estimate": "i:ipppp", "mgpu_host_wiener_tables": "i:ippiipppp",
    },
    "mercury_gpu.h": {
        "mgpu_create": "i:pp", "mgpu_create_explicit": "i:ppp", "mgpu_destroy": "v:p", "mgpu_last_error": "s:p", "mgpu_get_info": "i:pp",
        "mgpu_alloc_host": "p:z", "mgpu_free_host": "v:p", "mgpu_device_props_get": "i:ip", "mgpu_alloc_host_near": "p:iz",
        "mgpu_host_numa_node_of_pci": "i:s", "mgpu_host_numa_cpus": "i:ipi", "mgpu_rx_batch": "i:ppippp", "mgpu_rx_batch_taps": "i:ppippp",
        "mgpu_ldpc_batch": "i:ppipp", "mgpu_host_select_peak": "i:piiiiipp", "mgpu_host_fir_taps": "i:idpp", "mgpu_host_preamble_carriers": "i:ipp",
        "mgpu_host_mode_info": "i:iip", "mgpu_host_layout_stats": "i:ip", "mgpu_host_libm_selfcheck": "i:p", "mgpu_ldpc_encode_batch": "i:ppip",
        "mgpu_rx_batch_dev": "i:ppipppp", "mgpu_frontend_dev": "i:ppippp", "mgpu_ldpc_batch_dev": "i:ppipppppp", "mgpu_device_malloc": "p:pz",
        "mgpu_device_free": "v:pp", "mgpu_context_stream": "p:p", "mgpu_synchronize": "i:pp", "mgpu_copy_to_host": "i:pppzp",
        "mgpu_copy_to_device": "i:pppzp", "mgpu_txgen_dev": "i:puuidippp", "mgpu_baseband_test_esn0": "i:ppiquuip",
        "mgpu_passband_to_baseband": "i:ppiipipiip", "mgpu_time_sync_preamble": "i:ppiiiiipp", "mgpu_freq_sync": "i:ppiip",
        "mgpu_time_sync_mfsk": "i:ppiiip", "mgpu_detect_ack_pattern": "i:ppiiipp", "mgpu_detect_ack_pattern_from_passband": "i:ppiidipp",
        "mgpu_last_sync_kernel_ms": "i:pp", "mgpu_enable_timing": "i:pi", "mgpu_kernel_ms_avg": "i:ppp", "mgpu_decoder_hard_frames": "i:pp",
        "mgpu_host_path_last": "i:pppppp", "mgpu_last_kernel_ms": "i:pp", "mgpu_debug_mfsk_sync": "i:ppiiipip", "mgpu_debug_p2b_variant": "i:i",
        "mgpu_debug_span_energy": "i:ppiippiiipp", "mgpu_debug_spa_bins": "i:ipppp", "mgpu_debug_spa_math": "i:ppipp",
        "mgpu_debug_select_peak": "i:ppiipppiipp", "mgpu_debug_occupancy": "i:pi", "mgpu_debug_tsync_metric": "i:ppiiiippp",
        "mgpu_debug_glibc_trig": "i:ppippp",
    },
    "mercury_linksim.h": {
        "mgpu_linksim_create": "i:pppp", "mgpu_linksim_destroy": "i:p", "mgpu_linksim_run": "i:pippipp", "mgpu_linksim_counters_get": "i:pp",
        "mgpu_linksim_capture": "i:pp", "mgpu_linksim_noise_amp": "i:pp", "mgpu_host_linksim_frame_start": "i:piiiqp",
        "mgpu_host_linksim_payload": "i:uiqip",
    },
    "mercury_pool.h": {
        "mgpu_pool_create": "i:ppip", "mgpu_pool_destroy": "v:p", "mgpu_pool_size": "i:p", "mgpu_pool_device_numa_node": "i:pi",
        "mgpu_pool_context": "p:pi", "mgpu_pool_last_error": "s:p", "mgpu_pool_last_counters": "i:pp", "mgpu_pool_shard": "v:iiipp",
        "mgpu_pool_rx_batch": "i:ppipp", "mgpu_pool_ldpc_batch": "i:ppipp", "mgpu_pool_receive_byte_batch": "i:ppipppp",
        "mgpu_pool_rx_batch_dev": "i:ppppp", "mgpu_pool_ldpc_batch_dev": "i:ppppp", "mgpu_pool_txgen_dev": "i:puupdipp",
    },
    "mercury_rxloop.h": {
        "mgpu_receive_buffer_nsymb": "i:p", "mgpu_receive_byte_batch": "i:ppipppp", "mgpu_receive_byte_batch_samples": "i:ppiipppp",
        "mgpu_measure_signal_only": "i:ppidp", "mgpu_passband_test_esn0": "i:ppiquuddppp",
    },
    "mercury_shm.h": {
        "mgpu_shm_create": "i:szp", "mgpu_shm_connect": "i:szp", "mgpu_shm_close": "v:p", "mgpu_shm_destroy": "v:p", "mgpu_shm_used": "z:p",
        "mgpu_shm_free": "z:p", "mgpu_shm_capacity": "z:p", "mgpu_shm_clear": "v:p", "mgpu_shm_write": "i:ppz", "mgpu_shm_read": "i:ppz",
        "mgpu_shm_read_all": "l:pp", "mgpu_shm_publish_decoded": "i:pppiiipp",
    },
    "mercury_stages.h": {
        "mgpu_symbol_demod": "i:ppip", "mgpu_automatic_gain_control": "i:ppi", "mgpu_channel_estimator": "i:ppip",
        "mgpu_restore_channel_amplitude": "i:ppi", "mgpu_channel_equalizer": "i:pppip", "mgpu_measure_variance": "i:ppip", "mgpu_deframer": "i:ppip",
        "mgpu_deinterleaver_c128": "i:ppiiip", "mgpu_deinterleaver_f32": "i:ppiiip", "mgpu_psk_demod": "i:ppipp",
        "mgpu_bit_energy_dispersal": "i:ppiip", "mgpu_bit_to_byte": "i:ppiip", "mgpu_crc16_modbus_rtu": "i:ppiip",
    },
    "mercury_tx.h": {
        "mgpu_host_pre_equalization_channel": "i:idp", "mgpu_context_pre_equalization_channel": "i:pdp", "mgpu_set_pre_equalization_channel": "i:pp",
        "mgpu_transmit_frame_samples": "i:p", "mgpu_transmit_byte_batch": "i:ppipipp", "mgpu_transmit_bit_batch": "i:ppipp",
        "mgpu_transmit_byte_batch_dev": "i:ppipippp", "mgpu_transmit_buffer": "i:ppi", "mgpu_generate_ack_pattern_passband": "i:pipp",
        "mgpu_symbol_mod": "i:ppip",
    },
    "mercury_wiener_bank.h": {
        "mgpu_set_wiener_bank": "i:pipiz", "mgpu_get_wiener_bank": "i:pippz", "mgpu_get_wiener_choice": "i:piipppp",
        "mgpu_host_wiener_select": "i:ippizppppp", "mgpu_host_wiener_bank_thresholds": "i:ippizpp",
    },
}

# The ABI's extensions: headers under include/ext/, keyed by their path below include/. The set of prototypes under include/*.h is closed
# (tests/test_abi.py pins it); what the ABI gains later is declared here, typed by load_library() like the rest and checked against its
# header by tests/test_abi_extensions.py.
EXTENSIONS = {
    "ext/mercury_excisor.h": {
        "mgpu_set_excisor": "i:pipz", "mgpu_get_excisor": "i:pppz", "mgpu_get_excisor_report": "i:piip", "mgpu_excise_dev": "i:ppiidppp",
        "mgpu_host_excise": "i:pdpipp",
    },
    "ext/mercury_resampler.h": {
        "mgpu_resamp_create": "i:ppp", "mgpu_resamp_destroy": "i:p", "mgpu_resamp_info": "i:pp", "mgpu_resamp_seek": "i:pu",
        "mgpu_resamp_process": "i:ppiipzp", "mgpu_resamp_process_dev": "i:ppiipzpp", "mgpu_capture_run_resampled": "i:pppiippipp",
        "mgpu_host_resamp_design": "i:iiiddpp", "mgpu_host_resamp_default_taps": "i:iipp", "mgpu_host_resamp_process": "i:ppiiupzp",
        "mgpu_host_resamp_count": "i:iiuip",
    },
    "ext/mercury_synth.h": {
        "mgpu_synth_create": "i:pppp", "mgpu_synth_destroy": "i:p", "mgpu_synth_latency": "i:p", "mgpu_synth_seek": "i:pu",
        "mgpu_synth_retune": "i:pip", "mgpu_synth_process": "i:ppziip", "mgpu_synth_process_dev": "i:ppziipp", "mgpu_synth_status": "i:pp",
        "mgpu_host_synth_tables": "i:pppppp", "mgpu_host_synth_process": "i:pppziuipp",
    },
    "ext/mercury_scanner.h": {
        "mgpu_scan_create": "i:ppp", "mgpu_scan_destroy": "i:p", "mgpu_scan_seek": "i:pu", "mgpu_scan_lines": "i:pi",
        "mgpu_scan_process": "i:ppiippp", "mgpu_scan_process_dev": "i:ppiipppp", "mgpu_scan_status": "i:pp",
        "mgpu_host_scan_process": "i:ppiiuppp", "mgpu_host_scan_plan": "i:ppiip",
    },
    "ext/mercury_tuner.h": {
        "mgpu_tune_create": "i:pppp", "mgpu_tune_destroy": "i:p", "mgpu_tune_retune": "i:pip", "mgpu_tune_samples": "i:p",
        "mgpu_tune_process": "i:ppiip", "mgpu_tune_arrays": "i:pppp", "mgpu_host_tune_process": "i:pppiipppp",
        "mgpu_host_tune_plan": "i:ppp",
    },
    "ext/mercury_wideband_blanker.h": {
        "mgpu_wblank_create": "i:ppp", "mgpu_wblank_destroy": "i:p", "mgpu_wblank_seek": "i:pu", "mgpu_wblank_status": "i:pp",
        "mgpu_wblank_process": "i:ppippp", "mgpu_wblank_process_dev": "i:ppipppp", "mgpu_host_wblank_process": "i:ppiuppp",
    },
    "ext/mercury_iq_corrector.h": {
        "mgpu_iqc_create": "i:ppp", "mgpu_iqc_destroy": "i:p", "mgpu_iqc_seek": "i:pu", "mgpu_iqc_status": "i:pp",
        "mgpu_iqc_process": "i:ppippp", "mgpu_iqc_process_dev": "i:ppipppp", "mgpu_host_iqc_process": "i:ppiuppp",
        "mgpu_host_iqc_continue": "i:pppiuppp",
    },
}

# NOT ABI: exports that no header declares and that only tests and tools call (csrc/ctx.hpp, csrc/ldpc.hip). The one letter of
# their own is I, `unsigned` (a set of MGPU_FE_* form bits). A build that does not export one of them (the census and stamps hooks
# exist in variant builds only) goes without it.
NOT_ABI = {
    "mgpu_frontend_lds_bytes": "z:iiii", "mgpu_frontend_csi_lds_bytes": "z:iiii", "mgpu_frontend_nmap_lds_bytes": "z:iiii",
    "mgpu_frontend_wiener_lds_bytes": "z:iiiii", "mgpu_frontend_form_lds_bytes": "z:iiiiI", "mgpu_frontend_form_kernel": "p:iI",
    "mgpu_frontend_lds_workgroups": "i:z", "mgpu_debug_spa_census": "i:pi", "mgpu_debug_spa_stamps": "i:pi",
}

_CTYPES = {"i": C.c_int, "z": C.c_size_t, "u": C.c_uint64, "q": C.c_longlong, "d": C.c_double, "s": C.c_char_p, "p": C.c_void_p,
           "I": C.c_uint, "l": C.c_long, "v": None}


def prototype(signature):
    """"i:ppi" -> (restype, [argtypes])"""
    ret, _, params = signature.partition(":")
    return _CTYPES[ret], [_CTYPES[p] for p in params]


def names(*headers):
    """the functions the given headers declare, in the headers' order"""
    return [name for header in headers for name in (PROTOTYPES.get(header) or EXTENSIONS[header])]


_lib = None


def load_library():
    """dlopen the HIP library and give every function of the table its prototype; raise (never fall back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the Mercury RX path has no CPU fallback)" % LIB_PATH)
        # torch (used by bench/tests for device buffers, streams and torch.distributed) bundles its own
        # HIP runtime under the same SONAME; it has to be the first one in the process or the process ends
        # up with two HSA runtimes and the second one sees no GPU.
        try:
            import torch  # noqa: F401
        except Exception:  # torch is plumbing, not a dependency of the library itself
            pass
        lib = C.CDLL(LIB_PATH)
        missing = [name for name in names(*PROTOTYPES, *EXTENSIONS) if not hasattr(lib, name)]
        if missing:
            raise RuntimeError("%s does not export %s, which include/ declares" % (LIB_PATH, ", ".join(missing)))
        for group in list(PROTOTYPES.values()) + list(EXTENSIONS.values()) + [{n: s for n, s in NOT_ABI.items() if hasattr(lib, n)}]:
            for name, signature in group.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = prototype(signature)
        _lib = lib
    return _lib
