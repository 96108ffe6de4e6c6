"""wofdm_amd -- MI355X-native windowed-OFDM Monte-Carlo BER hot path.

The directory is named ``w-ofdm-optimization_amd`` (not an importable identifier); import it
as ``wofdm_amd`` through the shim module at the repository root.

  variants     structure table, raised-cosine / optimised window vectors  (host, numpy)
  simulation   run_simulation / wOFDMSystem / simulation_fun mirrors + Plan (ctypes -> HIP)
  distributed  frame-range sharding + counter all-reduce
  driver       main_BER_calculation.m / `-m run_sim` as functions, reference file formats
  channels     ITU-R tapped-delay-line channel realisations (gen_chan mirror)
  interference closed-form ICI+ISI power of a structure (interf_power mirror, host numpy)
  window_design  interference Hessians + QP -> optimised windows (optimizers.py / window_optimization.m)
  timefreq     Tx-side PSD / out-of-band-radiation estimate (timefreq_simulation.py)
  channel_mask main_channel_mask.m: half-band loading + spectral Tx mask (GPU: allocation / tx_mask)
  rx_profile   per-subcarrier BER / EVM of the frames the BER loop runs (GPU: wofdm_rx_profile; fp64 host mirror), alone or
               beside an asynchronous adjacent-band neighbour (GPU: wofdm_rx_profile_aci), or under receiver timing and
               carrier-frequency offset (GPU: wofdm_rx_profile_sync), or over channels that move within the frame
               (GPU: wofdm_rx_profile_doppler), or behind a nonlinear power amplifier (GPU: wofdm_rx_profile_pa; the
               spectral regrowth: timefreq / wofdm_tx_psd_batch_pa), or under oscillator phase noise (GPU:
               wofdm_rx_profile_pn), or with all five combined (GPU: wofdm_rx_profile_link), with soft decisions and the
               achievable rate beside the hard counters (GPU: wofdm_rx_profile_soft), behind a receiver that tracks with comb
               pilots and a postamble (GPU: wofdm_rx_profile_tracking), with 8-bit soft bits and a K = 7 Viterbi decoder behind
               it (GPU: wofdm_rx_profile_coded, wofdm_viterbi_decode), per data symbol or with one codeword over the frame (GPU:
               wofdm_rx_profile_coded_frame, wofdm_viterbi_decode_long), or with a quasi-cyclic LDPC code and a layered min-sum
               decoder over the frame (GPU: wofdm_rx_profile_ldpc, wofdm_ldpc_decode), or both decoders on random information
               words encoded on the GPU in the place of the all-zero word (GPU: wofdm_rx_profile_coset, wofdm_conv_encode,
               wofdm_ldpc_encode), or with retransmissions of the LDPC words and soft combining, up to the goodput per on-air
               sample (GPU: wofdm_rx_profile_harq, wofdm_ldpc_harq_decode)
  _lib         ctypes binding of libwofdm_hip.so (include/wofdm.h)
"""
from . import variants  # noqa: F401
from . import _lib  # noqa: F401
from . import distributed  # noqa: F401
from . import channels  # noqa: F401
from . import driver  # noqa: F401
from . import interference  # noqa: F401
from . import window_design  # noqa: F401
from . import timefreq  # noqa: F401
from . import channel_mask  # noqa: F401
from . import rx_profile  # noqa: F401
from .simulation import (Plan, ber_for_window_file, error_rates, make_cfg,  # noqa: F401
                         results_from_counts, run_counts, run_counts_injected, run_simulation,
                         save_ber_results, simulation_fun, wOFDMSystem)
from ._lib import kernel_source_hash  # noqa: F401
from .timefreq import (estimate_obr, frame_papr, papr_ccdf, papr_hist, run_timefreq, tx_papr_gpu,  # noqa: F401
                       tx_psd_batch_gpu, tx_waveform)
from .channel_mask import (aci_for_window_file, coded_for_window_file, coded_frame_for_window_file, coset_for_window_file, doppler_for_window_file, harq_for_window_file, interference_for_window_file,  # noqa: F401
                           ldpc_for_window_file,
                           link_for_window_file, soft_for_window_file, pa_for_window_file, papr_for_window_file, pn_for_window_file, profile_for_window_file,
                           spectrum_for_window_file, sync_for_window_file, tracking_for_window_file)
from .rx_profile import (RxProfile, RxProfileSync, SyncPoint, ber_per_bin, evm_db, frame_profile,  # noqa: F401
                         frame_profile_aci, frame_profile_sync, gen_noise_at, rx_profile_aci_gpu, rx_profile_aci_host,
                         rx_profile_gpu, rx_profile_host, rx_profile_sync_chunk_frames, rx_profile_sync_gpu,
                         rx_profile_sync_host, frame_profile_doppler, rx_profile_doppler_chunk_frames,
                         rx_profile_doppler_gpu, rx_profile_doppler_host, tv_conv,
                         PA_CLIP, PA_LINEAR, PA_RAPP, PaPoint, RxProfilePa, frame_profile_pa, pa_apply, pa_gain, pa_ref_power,
                         rx_profile_pa_chunk_frames, rx_profile_pa_gpu, rx_profile_pa_host,
                         PnPoint, frame_profile_pn, gen_pn_increments, pn_walk, rx_profile_pn_chunk_frames, rx_profile_pn_gpu,
                         rx_profile_pn_host,
                         LinkPoint, RxProfileLink, frame_profile_link, rx_profile_link_chunk_frames, rx_profile_link_gpu,
                         rx_profile_link_host,
                         RxProfileSoft, SOFT_SCALES, bit_llrs, frame_profile_soft, gmi, gmi_per_bin, gmi_per_symbol,
                         rx_profile_soft_chunk_frames, rx_profile_soft_gpu, rx_profile_soft_host, soft_penalties,
                         RxProfileTracking, TrackingPoint, frame_profile_tracking, pilot_comb, rx_profile_tracking_chunk_frames,
                         rx_profile_tracking_gpu, rx_profile_tracking_host, tracking_equalise,
                         CODE_RATES, LLR_SCALE, RxProfileCoded, code_steps, coded_ber, coded_cwer, conv_encode, default_interleaver,
                         frame_profile_coded, rx_profile_coded_chunk_frames, rx_profile_coded_gpu, rx_profile_coded_host, soft_bits,
                         viterbi_decode, viterbi_decode_gpu,
                         RxProfileCodedFrame, coded_fer, coded_frame_ber, default_sym_rot, frame_codewords, frame_interleaver,
                         frame_profile_coded_frame, rx_profile_coded_frame_chunk_frames, rx_profile_coded_frame_gpu,
                         rx_profile_coded_frame_host, viterbi_decode_long_gpu,
                         LDPC_MAX_ITER, RxProfileLdpc, frame_profile_ldpc, ldpc_ber, ldpc_decode, ldpc_decode_at, ldpc_decode_gpu,
                         ldpc_edges, ldpc_encode, ldpc_fer, ldpc_frame_words, ldpc_lift, ldpc_mean_iterations,
                         rx_profile_ldpc_chunk_frames, rx_profile_ldpc_gpu, rx_profile_ldpc_host,
                         STREAM_INFO, RxProfileCoset, conv_encode_gpu, coset_ber, coset_codewords, coset_fer, coset_info,
                         frame_profile_coset, ldpc_encode_gpu, rx_profile_coset_chunk_frames, rx_profile_coset_gpu,
                         rx_profile_coset_host,
                         RxProfileHarq, harq_acked, harq_bits_per_sample, harq_goodput, harq_mean_transmissions, harq_residual_fer,
                         harq_undetected, ldpc_harq_decode, ldpc_harq_decode_gpu, rx_profile_harq_chunk_frames, rx_profile_harq_gpu,
                         rx_profile_harq_host)
from .variants import (SYSTEMS, Structure, calculate_parameters, expand_rx_window,  # noqa: F401
                       expand_tx_window, make_structure, rx_rc_window, tx_rc_window)

__version__ = "0.1.0"
