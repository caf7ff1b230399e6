"""mercury_amd — MI355X-native implementation of Mercury's physical-layer RX hot path (and its transmit mirror).

Only what the path needs lives here: ``csrc/`` (hand-written HIP kernels for gfx950 + the C-ABI
declared in ``include/mercury_gpu.h``), ``data/`` (the LDPC graphs as compact derived data) and
``abi.py`` (the library's loader and the one table of its functions' prototypes), ``physical_layer.py`` (a ctypes binding mirroring
the reference's physical_layer surface), ``shm.py`` (the shared-memory ring decoded payloads are published through,
``include/mercury_shm.h``).
"""
from .physical_layer import (CAPTURE_SYMBOLS, DEC_GBF, DEC_MINSUM, DEC_SPA, DEC_SPA_FAST, EXPORTED_SYMBOLS, HF_CHANNEL_SYMBOLS, HF_PRESETS, LIB_PATH, HfChannel,
                             MgpuError, RxCapture, RxPhy, RxPool, STATS_DTYPE, device_props, hf_channel_preset, host_hf_channel_draws, host_hf_channel_taps,
                             host_hilbert_taps, load_library, pool_shard, HF_STREAM_SYMBOLS, LINKSIM_SYMBOLS, LINKSIM_COUNTERS_DTYPE, HfStream, LinkSim,
                             LinkSimConfig, linksim_config, host_hf_stream_noise, host_linksim_frame_start, host_linksim_payload, ESTIMATOR_SYMBOLS, LADDER_MAX, host_ls_estimate, parse_ladder, host_wiener_estimate, host_wiener_tables, WIENER_DESIGN_DEFAULT,
                             DIVERSITY_SYMBOLS, DIVERSITY_MAX, host_llr_combine, DEMAPPER_SYMBOLS, DEMAPPERS, host_demap_csi, host_demap_nmap, parse_demapper, NMAP_DEFAULT, DemapperParams,
                             CFO_SYMBOLS, CFO_MODES, host_cfo_pilots, BLANKER_SYMBOLS, BLANKER_MODES, BLANKER_DEFAULT, BLANKER_REPORT_DTYPE, BlankerParams, host_blank, parse_blanker,
                             WIENER_BANK_SYMBOLS, WIENER_BANK_MAX, WienerBankEntry, host_wiener_select, host_wiener_bank_thresholds, wiener_sounding, bank_entries,
                             CHANNELIZER_SYMBOLS, Channelizer, ChanChannel, ChanConfig, chan_channels, chan_config, host_chan_design, host_chan_tables, host_chan_process,
                             EXCISOR_SYMBOLS, EXCISOR_MODES, EXCISOR_DEFAULT, EXCISOR_REPORT_DTYPE, ExcisorParams, host_excise, parse_excisor,
                             RESAMPLER_SYMBOLS, Resampler, ResampConfig, ResampStatus, resamp_config, resamp_ratio, host_resamp_design, host_resamp_process,
                             host_resamp_count,
                             SYNTH_SYMBOLS, Synthesizer, SynthConfig, SynthState, synth_config, host_synth_process, host_synth_tables,
                             SCANNER_SYMBOLS, SCAN_MAX_RUNS, SCAN_DEFAULT_THRESHOLD, SCAN_REPORT_DTYPE, SCAN_RUN_DTYPE, BandScanner, ScanConfig, ScanState, scan_config,
                             scan_reports, host_scan_process, host_scan_plan,
                             TUNER_SYMBOLS, TUNE_DEFAULT_MIN_METRIC, TUNE_DEFAULT_CARRIER_HZ, TUNE_REPORT_DTYPE, Tuner, TuneConfig, tune_config, tune_samples,
                             tune_reports, host_tune_process, host_tune_plan,
                             WBLANK_SYMBOLS, WBLANK_DEFAULT_THRESHOLD, WBLANK_DEFAULT_GUARD, WBLANK_DEFAULT_MAX_SHARE, WBLANK_REPORT_DTYPE, WidebandBlanker,
                             WblankConfig, WblankState, wblank_config, wblank_block, wblank_reports, host_wblank_process,
                             IQC_SYMBOLS, IQC_DEFAULT_MEMORY, IQC_DEFAULT_BLOCK, IQC_SKIPPED, IQC_NO_BALANCE, IQC_REPORT_DTYPE, IqCorrector, IqcConfig,
                             IqcState, iqc_config, iqc_reports, iqc_image_db, host_iqc_process)

from .shm import ShmRing  # noqa: E402

__all__ = ["ShmRing", "RxPhy", "RxCapture", "CAPTURE_SYMBOLS", "RxPool", "pool_shard", "MgpuError", "DEC_GBF", "DEC_SPA", "DEC_MINSUM", "DEC_SPA_FAST", "STATS_DTYPE", "load_library",
           "LIB_PATH", "EXPORTED_SYMBOLS", "device_props", "HfChannel", "HF_PRESETS", "HF_CHANNEL_SYMBOLS", "hf_channel_preset", "host_hilbert_taps",
           "host_hf_channel_draws", "host_hf_channel_taps", "HfStream", "LinkSim", "LinkSimConfig", "linksim_config", "HF_STREAM_SYMBOLS", "LINKSIM_SYMBOLS",
           "LINKSIM_COUNTERS_DTYPE", "host_hf_stream_noise", "host_linksim_frame_start", "host_linksim_payload", "ESTIMATOR_SYMBOLS", "LADDER_MAX", "host_ls_estimate",
           "parse_ladder", "host_wiener_estimate", "host_wiener_tables", "WIENER_DESIGN_DEFAULT", "DIVERSITY_SYMBOLS", "DIVERSITY_MAX", "host_llr_combine", "DEMAPPER_SYMBOLS", "DEMAPPERS", "host_demap_csi", "host_demap_nmap", "parse_demapper", "NMAP_DEFAULT", "DemapperParams",
           "CFO_SYMBOLS", "CFO_MODES", "host_cfo_pilots", "BLANKER_SYMBOLS", "BLANKER_MODES", "BLANKER_DEFAULT", "BLANKER_REPORT_DTYPE", "BlankerParams", "host_blank", "parse_blanker",
           "WIENER_BANK_SYMBOLS", "WIENER_BANK_MAX", "WienerBankEntry", "host_wiener_select", "host_wiener_bank_thresholds", "wiener_sounding", "bank_entries",
           "CHANNELIZER_SYMBOLS", "Channelizer", "ChanChannel", "ChanConfig", "chan_channels", "chan_config", "host_chan_design", "host_chan_tables", "host_chan_process",
           "EXCISOR_SYMBOLS", "EXCISOR_MODES", "EXCISOR_DEFAULT", "EXCISOR_REPORT_DTYPE", "ExcisorParams", "host_excise", "parse_excisor",
           "RESAMPLER_SYMBOLS", "Resampler", "ResampConfig", "ResampStatus", "resamp_config", "resamp_ratio", "host_resamp_design", "host_resamp_process",
           "host_resamp_count",
           "SYNTH_SYMBOLS", "Synthesizer", "SynthConfig", "SynthState", "synth_config", "host_synth_process", "host_synth_tables",
           "SCANNER_SYMBOLS", "SCAN_MAX_RUNS", "SCAN_DEFAULT_THRESHOLD", "SCAN_REPORT_DTYPE", "SCAN_RUN_DTYPE", "BandScanner", "ScanConfig", "ScanState", "scan_config",
           "scan_reports", "host_scan_process", "host_scan_plan",
           "TUNER_SYMBOLS", "TUNE_DEFAULT_MIN_METRIC", "TUNE_DEFAULT_CARRIER_HZ", "TUNE_REPORT_DTYPE", "Tuner", "TuneConfig", "tune_config", "tune_samples",
           "tune_reports", "host_tune_process", "host_tune_plan",
           "WBLANK_SYMBOLS", "WBLANK_DEFAULT_THRESHOLD", "WBLANK_DEFAULT_GUARD", "WBLANK_DEFAULT_MAX_SHARE", "WBLANK_REPORT_DTYPE", "WidebandBlanker",
           "WblankConfig", "WblankState", "wblank_config", "wblank_block", "wblank_reports", "host_wblank_process",
           "IQC_SYMBOLS", "IQC_DEFAULT_MEMORY", "IQC_DEFAULT_BLOCK", "IQC_SKIPPED", "IQC_NO_BALANCE", "IQC_REPORT_DTYPE", "IqCorrector", "IqcConfig",
           "IqcState", "iqc_config", "iqc_reports", "iqc_image_db", "host_iqc_process"]
