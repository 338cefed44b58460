"""The C ABI of libtrxsig (include/trxsig*.h) as ctypes sees it, declared once: the structures the binding passes, one table
of every entry point's signature, and bind(), which _load applies to each library it opens.  tests/test_binding_abi.py holds
the table against the headers' prototypes and the structures against the C compiler's layout.  A new entry point gets one
line in SIGNATURES, beside its header's others, and nothing anywhere else."""
import ctypes as C


class TrxSigError(RuntimeError):
    pass


def _fields(ints, ptrs):
    return [(n, C.c_int) for n in ints] + [(n, C.c_void_p) for n in ptrs]


class C32(C.Structure):
    """By value."""
    _c_name_ = "trxsig_c32"
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


class TrxGroupResult(C.Structure):
    _c_name_ = "trxsig_trxgroup_result"
    _fields_ = _fields(("n_slots", "n_arfcn", "n_rows"), ("d_row", "d_valid", "d_flags", "d_amp", "d_toa", "d_avgpwr", "d_threshold",
                                                           "d_soft")) + [("soft_stride", C.c_int)]


class L1RxOut(C.Structure):
    _c_name_ = "trxsig_l1rx_out"
    _fields_ = _fields(("n_tch", "n_xcch", "nb_tch", "nb_xcch", "rach_cap"),
                       ("d_tch_status", "d_tch_frames", "d_facch", "d_tch_fer", "d_tch_fn", "d_xcch_status", "d_xcch_frames",
                        "d_xcch_fer", "d_xcch_fn", "d_rach_count", "d_rach_fn", "d_rach_arfcn", "d_rach_rssi", "d_rach_timing",
                        "d_rach_ok", "d_rach_ra", "d_tch_rssi", "d_tch_timing", "d_xcch_rssi", "d_xcch_timing", "d_ms_power", "d_ms_ta"))


class L1TxIn(C.Structure):
    _c_name_ = "trxsig_l1tx_in"
    _fields_ = _fields((), ("d_tch_kind", "d_tch_payload", "d_xcch_kind", "d_xcch_payload", "d_ccch_kind", "d_ccch_payload"))


class L1TxOut(C.Structure):
    _c_name_ = "trxsig_l1tx_out"
    _fields_ = _fields(("n_arfcn", "n_frames", "n_xcch"), ("d_bits", "d_what", "d_ms_power", "d_ms_ta"))


class L1MsIn(C.Structure):
    _c_name_ = "trxsig_l1ms_in"
    _fields_ = _fields((), ("d_tch_kind", "d_tch_payload", "d_xcch_kind", "d_xcch_payload", "d_rach_kind", "d_rach_ra", "d_rach_bsic"))


class L1MsOut(C.Structure):
    _c_name_ = "trxsig_l1ms_out"
    _fields_ = _fields(("n_arfcn", "n_frames", "n_xcch"), ("d_bits", "d_what", "d_ms_power", "d_ms_ta"))


class L1MsAir(C.Structure):
    _c_name_ = "trxsig_l1ms_air"
    _fields_ = _fields((), ("d_tch_gain", "d_tch_delay", "d_xcch_gain", "d_xcch_delay", "d_rach_gain", "d_rach_delay", "d_amp_of_power"))


class L1MsRxOut(C.Structure):
    _c_name_ = "trxsig_l1msrx_out"
    _fields_ = _fields(("n_tch", "n_xcch", "n_ccch", "n_bcch", "nb_tch", "nb_ctl", "sch_cap", "fcch_cap"),
                       ("d_tch_status", "d_tch_frames", "d_facch", "d_tch_fer", "d_tch_fn",
                        "d_xcch_status", "d_xcch_frames", "d_xcch_fer", "d_xcch_fn",
                        "d_ccch_status", "d_ccch_frames", "d_ccch_fer", "d_ccch_fn",
                        "d_bcch_status", "d_bcch_frames", "d_bcch_fer", "d_bcch_fn", "d_bcch_tc",
                        "d_sch_fn", "d_sch_rfn", "d_sch_present", "d_sch_ok", "d_sch_bsic", "d_sch_sync", "d_fcch_fn", "d_fcch_ones",
                        "d_tch_rssi", "d_tch_timing", "d_xcch_rssi", "d_xcch_timing", "d_ccch_rssi", "d_ccch_timing", "d_bcch_rssi",
                        "d_bcch_timing", "d_ord_power", "d_ord_ta"))


class L1AcqOut(C.Structure):
    _c_name_ = "trxsig_l1acq_out"
    _fields_ = _fields(("n_streams", "soft_stride"),
                       ("d_state", "d_fcch_k", "d_fcch_metric", "d_fcch_c", "d_fcch_e", "d_arg", "d_omega", "d_sch_w0", "d_sch_ptm",
                        "d_sch_amp", "d_sch_toa", "d_soft", "d_ok", "d_bsic", "d_rfn"))


class AirCellParams(C.Structure):
    _c_name_ = "trxsig_air_cell_params"
    _fields_ = [("d_taps", C.c_void_p), ("n_taps", C.c_int), ("d_step", C.c_void_p), ("d_phase", C.c_void_p), ("d_sigma", C.c_void_p)]


class AirStreamParams(C.Structure):
    _c_name_ = "trxsig_air_stream_params"
    _fields_ = _fields(("n_arfcn",), ("d_arfcn", "d_cut", "d_delay", "d_step", "d_phase", "d_gain", "d_sigma", "d_n0"))


class L1TrkView(C.Structure):
    _c_name_ = "trxsig_l1trk_view"
    _fields_ = _fields(("n_phones", "n_cols"), ("d_fn", "d_pos", "d_phase", "d_step", "d_locked", "d_quiet", "d_toa_sum", "d_toa_n",
                                                "d_adj", "d_afc_n", "d_afc_delta"))


class L1TrkMeas(C.Structure):
    _c_name_ = "trxsig_l1trk_meas"
    _fields_ = _fields(("n_phones", "n_cols", "n_fcch", "fcch_stride"), ("d_status", "d_fcch_fn", "d_fcch_c", "d_fcch_e", "d_fcch_ok"))


vp, i32, u32, i64, u64, f32, f64, size, cstr, P = (C.c_void_p, C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double,
                                                   C.c_size_t, C.c_char_p, C.POINTER)

# name -> (restype, argtypes), in the headers' order.  A pointer is c_void_p unless the binding passes byref() of something typed.
SIGNATURES = {
    # ---- include/trxsig.h ----
    "trxsig_abi_version": (i32, []),
    "trxsig_create": (i32, [P(vp), i32, i32]),
    "trxsig_destroy": (None, [vp]),
    "trxsig_sps": (i32, [vp]),
    "trxsig_device": (i32, [vp]),
    "trxsig_live_children": (i32, [vp]),
    "trxsig_set_stream": (i32, [vp, vp]),
    "trxsig_synchronize": (i32, [vp]),
    "trxsig_get_stream": (vp, [vp]),
    "trxsig_get_device": (i32, [vp]),
    "trxsig_last_error": (cstr, [vp]),
    "trxsig_reserve": (i32, [vp, i32]),
    "trxsig_tables_bytes": (size, [i32]),
    "trxsig_tables_build_host": (i32, [i32, vp, size]),
    "trxsig_tables_device": (vp, [vp]),
    "trxsig_create_from_tables": (i32, [P(vp), i32, vp, size]),
    "trxsig_tables_export": (i32, [vp, vp, size]),
    "trxsig_tables_view_get": (i32, [vp, vp]),
    "trxsig_detect_demod_normal_batch": (i32, [vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_detect_demod_rach_batch": (i32, [vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_demodulate_batch": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_set_soft_mode": (i32, [vp, i32]),
    "trxsig_get_soft_mode": (i32, [vp]),
    "trxsig_mlse_batch": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_normal_batch": (i32, [vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_access_batch": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_rach_batch": (i32, [vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_access_pinv_host": (i32, [vp]),
    "trxsig_mlse_sch_batch": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_sch_pinv_host": (i32, [vp]),
    "trxsig_sch_fit_batch": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "trxsig_mlse_div_batch": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_div_normal_batch": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_irc_batch": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_mlse_irc_normal_batch": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_modulate_batch": (i32, [vp, vp, vp, vp, i32, vp, vp]),
    "trxsig_estimate_dfe_batch": (i32, [vp, vp, vp, vp, i32, i32, f32, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "trxsig_equalize_taps_batch": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_channel_estimate_batch": (i32, [vp, vp, vp, vp, i32, i32, f32, i32, i32, vp, vp, vp, vp, vp]),
    "trxsig_design_dfe_batch": (i32, [vp, vp, vp, vp, i32, vp, vp]),
    "trxsig_channel_estimate_host": (i32, [vp, vp, i32, i32, f32, i32, i32, vp, vp, vp, vp, vp]),
    "trxsig_design_dfe_host": (i32, [vp, vp, f32, vp, vp]),
    "trxsig_equalize_taps_host": (i32, [vp, vp, i32, C32, f32, vp, vp, vp, i32]),
    "trxsig_resample_batch": (i32, [vp, vp, i32, i64, i32, i32, i32, vp, i32, vp, i64]),
    "trxsig_resample_out_len": (i32, [i32, i32, i32]),
    "trxsig_resample_host": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, i32]),
    "trxsig_unpack_int16": (i32, [vp, vp, i64, i32, vp]),
    "trxsig_pack_int16": (i32, [vp, vp, i64, vp]),
    "trxsig_pack_int16_scaled": (i32, [vp, vp, i64, f32, vp]),
    "trxsig_unpack_half": (i32, [vp, vp, i64, vp]),
    "trxsig_equalize_normal_batch": (i32, [vp, vp, vp, vp, i32, i32, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_equalize_normal_batch_fmt": (i32, [vp, vp, i32, vp, vp, i32, i32, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_equalize_taps_batch_fmt": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_detect_demod_normal_host": (i32, [vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_detect_demod_rach_host": (i32, [vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_demodulate_host": (i32, [vp, vp, i32, C32, f32, vp, i32]),
    "trxsig_modulate_host": (i32, [vp, vp, vp, vp, i32, vp, vp, i64]),
    "trxsig_fec_xcch_decode_batch": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "trxsig_fec_rach_decode_batch": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    "trxsig_fec_xcch_encode_batch": (i32, [vp, vp, i32, i32, vp]),
    "trxsig_fec_tch_decode_batch": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "trxsig_fec_viterbi_batch": (i32, [vp, vp, i32, i64, i32, vp, i64]),
    "trxsig_fec_pdtch_encode_batch": (i32, [vp, vp, vp, vp, i32, vp]),
    "trxsig_fec_pdtch_decode_batch": (i32, [vp, vp, i32, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "trxsig_pdch_map_host": (i32, [i32, P(i32), P(i32)]),
    "trxsig_fec_access_encode_batch": (i32, [vp, vp, vp, vp, i32, vp]),
    "trxsig_fec_access_decode_batch": (i32, [vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "trxsig_fec_tch_decode_stream": (i32, [vp, i32, i32, vp, i32, i64, vp, vp, i32, vp, vp, vp, vp, vp]),
    "trxsig_fec_xcch_decode_stream": (i32, [vp, i32, i32, vp, i32, i64, vp, i32, vp, vp, vp, vp]),
    "trxsig_fec_tch_set_filler": (i32, [vp, vp]),
    "trxsig_fec_tch_encode_batch": (i32, [vp, i32, i32, vp, vp, vp, vp, vp]),
    "trxsig_fec_sch_encode_batch": (i32, [vp, vp, vp, i32, vp]),
    "trxsig_fec_sch_decode_batch": (i32, [vp, vp, i32, i32, vp, vp, vp]),
    "trxsig_convolve_out_len": (i32, [i32, i32, i32, i32]),
    "trxsig_convolve_batch": (i32, [vp, vp, vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "trxsig_convolve_host": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, i32]),
    "trxsig_delay_vector_batch": (i32, [vp, vp, vp, vp, i32, vp, i32, vp]),
    "trxsig_delay_vector_host": (i32, [vp, vp, i32, f32, i32]),
    "trxsig_interpolate_point_batch": (i32, [vp, vp, vp, vp, i32, vp, i32, vp]),
    "trxsig_interpolate_point_host": (i32, [vp, vp, i32, f32, i32, vp]),
    "trxsig_peak_detect_batch": (i32, [vp, vp, vp, vp, i32, vp, vp, vp]),
    "trxsig_peak_detect_host": (i32, [vp, vp, i32, vp, vp, vp]),
    "trxsig_energy_detect_batch": (i32, [vp, vp, vp, vp, i32, u32, i32, f32, vp, vp]),
    "trxsig_energy_detect_host": (i32, [vp, vp, i32, u32, i32, f32, vp]),
    "trxsig_scale_vector_batch": (i32, [vp, vp, vp, vp, i32, i32, vp, i32]),
    "trxsig_gmsk_rotate_batch": (i32, [vp, vp, vp, vp, i32, i32, i32, i32]),
    "trxsig_vector_slicer_batch": (i32, [vp, vp, vp, vp, i32, i32]),
    "trxsig_decimate_batch": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "trxsig_db": (f32, [f32]),
    "trxsig_dbinv": (f32, [f32]),
    "trxsig_sinc_host": (i32, [vp, f32, P(f32)]),
    "trxsig_gaussian_noise_host": (i32, [i32, f32, C32, vp]),
    "trxsig_vector_norm2_batch": (i32, [vp, vp, vp, vp, i32, vp, vp]),
    "trxsig_vector_norm2_host": (i32, [vp, vp, i32, P(f32), P(f32)]),
    "trxsig_frequency_shift_batch": (i32, [vp, vp, vp, vp, i32, vp, vp, i32, vp, vp]),
    "trxsig_frequency_shift_host": (i32, [vp, vp, i32, f32, f32, i32, vp, P(f32)]),
    "trxsig_add_vector_batch": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32]),
    "trxsig_add_vector_host": (i32, [vp, vp, i32, vp, i32]),
    "trxsig_offset_vector_batch": (i32, [vp, vp, vp, vp, i32, i32, vp, i32]),
    "trxsig_resample_linear_out_len": (i32, [i32, f32]),
    "trxsig_resample_linear_batch": (i32, [vp, vp, vp, vp, i32, f32, vp, vp, vp]),
    "trxsig_resample_linear_host": (i32, [vp, vp, i32, f32, C32, vp, i32]),
    "trxsig_elementwise_host": (i32, [vp, i32, vp, i32, C32, i32]),
    "trxsig_decimate_host": (i32, [vp, vp, i32, i32, vp]),
    "trxsig_timer_start": (i32, [vp]),
    "trxsig_timer_stop": (i32, [vp, P(f32)]),
    "trxsig_kernel_name": (cstr, [i32]),
    "trxsig_profile_enable": (i32, [vp, i32]),
    "trxsig_profile_collect": (i32, [vp, P(f32), P(i32)]),
    "trxsig_profile_collect_n": (i32, [vp, i32, P(f32), P(i32)]),
    "trxsig_kernel_count": (i32, []),
    "trxsig_set_tuning": (i32, [vp, i32, i32]),
    "trxsig_tuning_build": (i32, []),
    "trxsig_tables_validate_host": (i32, [vp, size]),
    "trxsig_tables_broadcast": (i32, [vp, vp, size, i32, vp]),
    "trxsig_tables_rach_error_bound": (i32, [vp, size, vp, vp]),
    # ---- include/trxsig_transceiver.h ----
    "trxsig_trx_create": (i32, [P(vp), i32, i32, i32, i32]),
    "trxsig_trx_set_tsc_leg": (i32, [vp, i32]),
    "trxsig_trx_destroy": (None, [vp]),
    "trxsig_trx_last_error": (cstr, [vp]),
    "trxsig_trx_context": (vp, [vp]),
    "trxsig_trx_control": (i32, [vp, cstr, cstr, i32]),
    "trxsig_trx_expected_corr_type": (i32, [vp, i32, i32]),
    "trxsig_trx_pull_radio_vector": (i32, [vp, vp, i32, i32, i32, vp, P(i32), P(i32), P(i32)]),
    "trxsig_trx_encode_rx_datagram": (i32, [i32, i32, i32, i32, vp, i32, vp]),
    "trxsig_trx_decode_tx_datagram": (i32, [vp, i32, P(i32), P(i32), P(i32), vp]),
    "trxsig_trx_add_radio_vector": (i32, [vp, vp, i32, i32, i32]),
    "trxsig_trx_push_radio_vector": (i32, [vp, i32, i32, vp, P(i32), P(i32)]),
    "trxsig_trx_energy_threshold": (f64, [vp]),
    "trxsig_trx_filler_modulus": (i32, [vp, i32]),
    "trxsig_trx_queue_size": (i32, [vp]),
    "trxsig_txclock_init": (None, [vp, i32, i32, i32, i32]),
    "trxsig_txclock_advance": (i32, [vp, i32, i32, vp, i32, vp, vp]),
    "trxsig_txclock_indication_due": (i32, [vp]),
    "trxsig_txclock_indication": (i32, [vp, vp, i32]),
    "trxsig_create_lpf_host": (i32, [vp, i32, f32, vp]),
    # ---- include/trxsig_trxgroup.h ----
    "trxsig_trxgroup_create": (i32, [P(vp), vp, i32, i32, i32, i32]),
    "trxsig_trxgroup_destroy": (None, [vp]),
    "trxsig_trxgroup_arfcns": (i32, [vp]),
    "trxsig_trxgroup_control": (i32, [vp, i32, cstr, cstr, i32]),
    "trxsig_trxgroup_expected_corr_type": (i32, [vp, i32, i32, i32]),
    "trxsig_trxgroup_pull": (i32, [vp, vp, i64, i64, i32, i32, i32, i32, P(TrxGroupResult)]),
    "trxsig_trxgroup_pull_rxfe": (i32, [vp, vp, vp, i32, i32, P(i32), P(TrxGroupResult)]),
    "trxsig_trxgroup_pull_bursts": (i32, [vp, vp, vp, vp, i32, i32, i32, P(TrxGroupResult)]),
    "trxsig_trxgroup_combine_div": (i32, [vp, vp, vp, vp, vp, vp, vp, P(TrxGroupResult)]),
    "trxsig_trxgroup_combine_irc": (i32, [vp, vp, vp, vp, f32, vp, vp, vp, vp, P(TrxGroupResult)]),
    "trxsig_trxgroup_collect": (i32, [vp, vp, vp, vp, vp, vp]),
    "trxsig_trxgroup_pull_host": (i32, [vp, vp, i64, i64, i32, i32, i32, i32]),
    "trxsig_trxgroup_set_pipelined": (i32, [vp, i32]),
    "trxsig_trxgroup_set_beside_rows": (i32, [vp, i32]),
    "trxsig_trxgroup_set_rach_leg": (i32, [vp, i32]),
    "trxsig_trxgroup_set_split_rows": (i32, [vp, i32]),
    "trxsig_trxgroup_sync": (i32, [vp]),
    "trxsig_trxgroup_energy_threshold": (i32, [vp, i32, P(f64)]),
    "trxsig_trxgroup_add_bursts": (i32, [vp, vp, vp, i32]),
    "trxsig_trxgroup_tx_staging": (i32, [vp, i32, P(vp), P(vp)]),
    "trxsig_trxgroup_add_staged": (i32, [vp, i32]),
    "trxsig_trxgroup_push": (i32, [vp, i32, i32, i32, P(vp), P(vp), P(vp)]),
    "trxsig_trxgroup_push_txbe": (i32, [vp, vp, i32, i32, i32]),
    "trxsig_trxgroup_tx_queue_size": (i32, [vp, i32, P(i32)]),
    # ---- include/trxsig_frontend.h ----
    "trxsig_rxfe_create": (i32, [P(vp), vp, i32, i32, vp, i32, i32, i32]),
    "trxsig_rxfe_destroy": (None, [vp]),
    "trxsig_rxfe_push": (i32, [vp, vp, i32]),
    "trxsig_rxfe_pop": (i32, [vp, P(vp), P(vp), P(vp), vp, i32, P(i32)]),
    "trxsig_rxfe_pending": (i32, [vp]),
    "trxsig_rxfe_push_detect_demod_normal": (i32, [vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, i32, i32, vp, i32, P(i32)]),
    "trxsig_rxfe_create_wideband": (i32, [P(vp), vp, i32, i32, vp, i32, i32, vp, i32, i32, i32]),
    "trxsig_rxfe_push_wideband": (i32, [vp, vp, i32]),
    "trxsig_rxfe_set_shared_filter": (i32, [vp, i32]),
    "trxsig_txbe_create": (i32, [P(vp), vp, i32, i32, vp, i32, f32]),
    "trxsig_txbe_set_fused": (i32, [vp, i32]),
    "trxsig_txbe_destroy": (None, [vp]),
    "trxsig_txbe_push_bursts": (i32, [vp, vp, vp, vp, i32]),
    "trxsig_txbe_can_push": (i32, [vp, vp, i32]),
    "trxsig_txbe_streams": (i32, [vp]),
    "trxsig_txbe_pop": (i32, [vp, P(vp), P(i64), P(i32)]),
    "trxsig_txbe_pending": (i32, [vp]),
    "trxsig_txbe_create_wideband": (i32, [P(vp), vp, i32, i32, vp, i32, i32, vp, i32, f32]),
    # ---- include/trxsig_l1rx.h ----
    "trxsig_l1rx_create": (i32, [P(vp), vp, i32, vp, i32, i32]),
    "trxsig_l1rx_destroy": (None, [vp]),
    "trxsig_l1rx_channels": (i32, [vp, i32]),
    "trxsig_l1rx_channel": (i32, [vp, i32, i32, P(i32), P(i32), P(i32), P(i32)]),
    "trxsig_l1rx_open": (i32, [vp, i32, i32]),
    "trxsig_l1rx_close": (i32, [vp, i32, i32]),
    "trxsig_l1rx_decode": (i32, [vp, P(TrxGroupResult), i32, i32, P(L1RxOut)]),
    "trxsig_l1rx_state": (i32, [vp, i32, P(vp)]),
    # ---- include/trxsig_l1tx.h ----
    "trxsig_l1tx_create": (i32, [P(vp), vp, i32, vp, i32, i32, f32]),
    "trxsig_l1tx_destroy": (None, [vp]),
    "trxsig_l1tx_channels": (i32, [vp, i32]),
    "trxsig_l1tx_channel": (i32, [vp, i32, i32, P(i32), P(i32), P(i32), P(i32)]),
    "trxsig_l1tx_open": (i32, [vp, i32, i32]),
    "trxsig_l1tx_close": (i32, [vp, i32, i32]),
    "trxsig_l1tx_set_si": (i32, [vp, vp]),
    "trxsig_l1tx_grid": (i32, [vp, i32, i32, P(i32), P(i32), P(i32)]),
    "trxsig_l1tx_encode": (i32, [vp, i32, i32, P(L1TxIn), vp, P(L1TxOut)]),
    "trxsig_l1tx_datagrams": (i32, [vp, vp, vp, i32, P(i32)]),
    "trxsig_trxgroup_add_l1tx": (i32, [vp, vp]),
    "trxsig_l1tx_state": (i32, [vp, i32, P(vp)]),
    # ---- include/trxsig_l1ms.h ----
    "trxsig_l1ms_create": (i32, [P(vp), vp, i32, vp, i32, i32]),
    "trxsig_l1ms_destroy": (None, [vp]),
    "trxsig_l1ms_channels": (i32, [vp, i32]),
    "trxsig_l1ms_channel": (i32, [vp, i32, i32, P(i32), P(i32), P(i32), P(i32)]),
    "trxsig_l1ms_open": (i32, [vp, i32, i32]),
    "trxsig_l1ms_close": (i32, [vp, i32, i32]),
    "trxsig_l1ms_set_phy": (i32, [vp, i32, i32, i32]),
    "trxsig_l1ms_grid": (i32, [vp, i32, i32, P(i32), P(i32), P(i32)]),
    "trxsig_l1ms_encode": (i32, [vp, i32, i32, P(L1MsIn), vp, P(L1MsOut)]),
    "trxsig_l1ms_radiate": (i32, [vp, P(L1MsAir), vp, i64, i64]),
    "trxsig_l1ms_state": (i32, [vp, i32, P(vp)]),
    "trxsig_l1ms_follow": (i32, [vp, vp]),
    # ---- include/trxsig_l1msrx.h ----
    "trxsig_l1msrx_create": (i32, [P(vp), vp, i32, vp, i32, i32]),
    "trxsig_l1msrx_destroy": (None, [vp]),
    "trxsig_l1msrx_channels": (i32, [vp, i32]),
    "trxsig_l1msrx_channel": (i32, [vp, i32, i32, P(i32), P(i32), P(i32), P(i32)]),
    "trxsig_l1msrx_open": (i32, [vp, i32, i32]),
    "trxsig_l1msrx_close": (i32, [vp, i32, i32]),
    "trxsig_l1msrx_decode": (i32, [vp, P(TrxGroupResult), i32, i32, P(L1MsRxOut)]),
    "trxsig_l1msrx_state": (i32, [vp, i32, P(vp)]),
    # ---- include/trxsig_l1acq.h ----
    "trxsig_l1acq_create": (i32, [P(vp), vp, i32, i32]),
    "trxsig_l1acq_destroy": (None, [vp]),
    "trxsig_l1acq_search": (i32, [vp, vp, i64, i32, i32, f32, f32, P(L1AcqOut)]),
    "trxsig_l1acq_detect_sch_batch": (i32, [vp, vp, vp, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp, i32]),
    "trxsig_l1acq_sequence": (i32, [vp, vp, vp, vp]),
    "trxsig_l1acq_set_sch_leg": (i32, [vp, i32]),
    "trxsig_l1acq_sch_channel": (i32, [vp, P(vp), P(vp)]),
    "trxsig_l1acq_set_sch_detector": (i32, [vp, i32]),
    "trxsig_l1acq_sch_fit": (i32, [vp, P(vp), P(vp)]),
    # ---- include/trxsig_air.h ----
    "trxsig_air_create": (i32, [P(vp), vp, i32]),
    "trxsig_air_destroy": (None, [vp]),
    "trxsig_air_cells": (i32, [vp, i32, i32, i32, u64, vp, i64, i64, P(AirCellParams), vp, i64, i64, i32]),
    "trxsig_air_stream": (i32, [vp, i32, u64, vp, i64, i64, i32, P(AirStreamParams), i32, vp, i64]),
    "trxsig_air_fade_profile": (i32, [vp, i32, vp, vp, vp, vp, i32, i32, i32]),
    "trxsig_air_fade_columns": (i32, [vp, i32, vp]),
    "trxsig_air_fade": (i32, [vp, i32, i32, i32, u64, vp, i32, vp, vp]),
    "trxsig_air_fade_params": (i32, [vp, u64, i32, vp, vp, vp]),
    # ---- include/trxsig_l1trk.h ----
    "trxsig_l1trk_create": (i32, [P(vp), vp, i32, i32, vp, vp, i32, i32, i32, f32]),
    "trxsig_l1trk_destroy": (None, [vp]),
    "trxsig_l1trk_seed": (i32, [vp, P(L1AcqOut), vp]),
    "trxsig_l1trk_set": (i32, [vp, i32, i32, i32, i64, u32, u32]),
    "trxsig_l1trk_state": (i32, [vp, P(L1TrkView)]),
    "trxsig_l1trk_slice": (i32, [vp, vp, i64, i64, i32, i32, i32, vp, i64, i64, P(L1TrkMeas)]),
    "trxsig_l1trk_update": (i32, [vp, P(TrxGroupResult), i32, vp]),
    # ---- include/trxsig_l1ciph.h ----
    "trxsig_a5_1_blocks_batch": (i32, [vp, i32, vp, vp, vp, vp]),
    "trxsig_l1ciph_create": (i32, [P(vp), vp, i32, vp]),
    "trxsig_l1ciph_destroy": (None, [vp]),
    "trxsig_l1ciph_channels": (i32, [vp, i32]),
    "trxsig_l1ciph_channel": (i32, [vp, i32, i32, P(i32), P(i32), P(i32), P(i32)]),
    "trxsig_l1ciph_set": (i32, [vp, i32, i32, i32, vp]),
    "trxsig_l1ciph_state": (i32, [vp, i32, P(vp)]),
    "trxsig_l1ciph_bits": (i32, [vp, i32, i32, i32, vp, vp, u32]),
    "trxsig_l1ciph_soft": (i32, [vp, i32, P(TrxGroupResult), i32]),
    # ---- include/trxsig_l1hop.h ----
    "trxsig_hop_mai_batch": (i32, [vp, i32, vp, vp, vp, vp, vp]),
    "trxsig_l1hop_create": (i32, [P(vp), vp, i32, vp, vp, i32, vp, i32]),
    "trxsig_l1hop_destroy": (None, [vp]),
    "trxsig_l1hop_groups": (i32, [vp]),
    "trxsig_l1hop_members": (i32, [vp, i32, i32, vp]),
    "trxsig_l1hop_map": (i32, [vp, i32, i32, P(vp)]),
    "trxsig_l1hop_bits": (i32, [vp, i32, i32, i32, vp, vp]),
    "trxsig_l1hop_cells": (i32, [vp, i32, i32, i32, vp, i64, i64, vp, i64, i64]),
    "trxsig_l1hop_result": (i32, [vp, i32, P(TrxGroupResult), P(TrxGroupResult)]),
    # ---- include/trxsig_l1pdch.h ----
    "trxsig_l1pdch_create": (i32, [P(vp), vp, i32, vp, i32, i32]),
    "trxsig_l1pdch_destroy": (None, [vp]),
    "trxsig_l1pdch_channels": (i32, [vp, i32]),
    "trxsig_l1pdch_channel": (i32, [vp, i32, i32, P(i32), P(i32)]),
    "trxsig_l1pdch_grid": (i32, [vp, i32, i32, P(i32), P(i32)]),
    "trxsig_l1pdch_state": (i32, [vp, i32, P(vp)]),
    "trxsig_l1pdch_encode": (i32, [vp, i32, i32, vp, vp, vp, vp]),
    "trxsig_l1pdch_decode": (i32, [vp, P(TrxGroupResult), i32, i32, i32, vp, vp]),
    # ---- include/trxsig_l1pacc.h ----
    "trxsig_l1pacc_create": (i32, [P(vp), vp, i32, vp, i32]),
    "trxsig_l1pacc_destroy": (None, [vp]),
    "trxsig_l1pacc_channels": (i32, [vp]),
    "trxsig_l1pacc_channel": (i32, [vp, i32, P(i32), P(i32)]),
    "trxsig_l1pacc_grid": (i32, [vp, i32, i32, P(i32)]),
    "trxsig_l1pacc_state": (i32, [vp, P(vp)]),
    "trxsig_l1pacc_encode": (i32, [vp, i32, i32, vp, vp, vp, vp]),
    "trxsig_l1pacc_detect": (i32, [vp, vp, i64, i64, i32, i32, vp, i32, i32, f32, f32, i32, vp]),
    "trxsig_l1pacc_ta_message": (i32, [vp, vp, vp, i32]),
    "trxsig_l1pacc_ta_read": (i32, [vp, vp, vp]),
}


def bind(cdll, path):
    """Type every entry point of a loaded library; a library without one of them is not this ABI and does not load."""
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            f = getattr(cdll, name)
        except AttributeError:
            raise TrxSigError("%s has no symbol %s, which include/trxsig*.h declares" % (path, name)) from None
        f.restype, f.argtypes = restype, argtypes
    return cdll
