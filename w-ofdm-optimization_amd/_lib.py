"""ctypes binding of libwofdm_hip.so (include/wofdm.h).

There is no CPU fallback: if the library is missing or no gfx950 device is usable,
the calls raise.  torch is not needed here -- device pointers are plain integers
(e.g. ``tensor.data_ptr()``), streams are raw ``hipStream_t`` values.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WOFDM_LIB: developer override for A/B builds of the same ABI (never a different backend)
LIB_PATH = os.environ.get("WOFDM_LIB", os.path.join(_HERE, "libwofdm_hip.so"))
_LIB = None

WOFDM_OK = 0
ERRORS = {-1: "WOFDM_E_INVALID", -2: "WOFDM_E_UNSUPPORTED", -3: "WOFDM_E_HIP", -4: "WOFDM_E_NOMEM"}
MAX_TAPS = 21
#: wofdm_plan_set_option: diagnostic kernel choice (include/wofdm.h)
OPTIONS = {"fir_valu": 0, "max_spw": 1, "txmask_direct": 2, "dft_valu": 3, "generic_geometry": 4}
MAX_SYMS = 16
#: wofdm_tx_papr (include/wofdm.h): device-memory budget of a chunk of frames, most periods the `periods` output takes
TX_PAPR_CHUNK_BYTES = 256 << 20
TX_PAPR_MAX_PERIODS = 1 << 20
#: wofdm_rx_profile (include/wofdm.h): device-memory budget of a chunk of frames
RX_PROFILE_CHUNK_BYTES = 256 << 20
#: wofdm_rx_profile_sync (include/wofdm.h): most points one call takes
SYNC_MAX_POINTS = 64
#: wofdm_rx_profile_doppler (include/wofdm.h): most tracks one call takes, most knots a track has
DOPPLER_MAX_TRACKS = 16
DOPPLER_MAX_KNOTS = 64
#: wofdm_rx_profile_pa, wofdm_tx_psd_batch_pa (include/wofdm.h): the amplifier models, most points one call takes
PA_LINEAR, PA_RAPP, PA_CLIP = 0, 1, 2
PA_MAX_POINTS = 16
#: wofdm_rx_profile_pn (include/wofdm.h): most points one call takes
PN_MAX_POINTS = 16
#: wofdm_rx_profile_link (include/wofdm.h): most points one call takes
LINK_MAX_POINTS = 16
#: wofdm_rx_profile_soft (include/wofdm.h): most scales one call takes
SOFT_MAX_SCALES = 16
#: wofdm_rx_profile_coded, wofdm_viterbi_decode (include/wofdm.h): most codes one call takes, most steps of a codeword
CODE_MAX = 4
CODE_MAX_STEPS = 4608
#: wofdm_viterbi_decode_long, wofdm_rx_profile_coded_frame (include/wofdm.h): most steps of a codeword
CODE_LONG_MAX_STEPS = 1048576
#: wofdm_ldpc_decode, wofdm_rx_profile_ldpc (include/wofdm.h): most positions of a codeword
LDPC_MAX_BITS = 16384
#: wofdm_coset_info, wofdm_rx_profile_coset (csrc/wofdm_link.h): the Philox stream of the information words
STREAM_INFO = 4

#: wofdm_rx_profile_harq, wofdm_ldpc_harq_decode (include/wofdm.h): most transmissions of a word, counters per code
HARQ_MAX_ROUNDS = 8
HARQ_FIELDS = 13

#: every symbol include/wofdm.h declares (tests check the .so exports them all)
EXPORTS = (
    "wofdm_version", "wofdm_device_count", "wofdm_last_error", "wofdm_noise_len",
    "wofdm_plan_create", "wofdm_plan_destroy", "wofdm_plan_launch", "wofdm_plan_launch_timed",
    "wofdm_plan_launch_injected", "wofdm_plan_dump_frame", "wofdm_plan_info", "wofdm_run",
    "wofdm_run_injected", "wofdm_philox_kat", "wofdm_plan_set_allocation",
    "wofdm_plan_set_tx_mask", "wofdm_plan_status", "wofdm_plan_kernel_id", "wofdm_plan_set_option",
    "wofdm_interference", "wofdm_tx_psd", "wofdm_tx_psd_batch", "wofdm_tx_psd_batch_masked",
    "wofdm_interference_masked", "wofdm_tx_papr", "wofdm_tx_papr_kernel_ms",
    "wofdm_rx_profile", "wofdm_rx_profile_kernel_ms", "wofdm_plan_kernel_geo", "wofdm_cfg_geo_id",
    "wofdm_rx_profile_aci", "wofdm_rx_profile_sync", "wofdm_rx_profile_doppler",
    "wofdm_rx_profile_pa", "wofdm_tx_psd_batch_pa", "wofdm_rx_profile_pn",
    "wofdm_rx_profile_link", "wofdm_rx_profile_soft", "wofdm_rx_profile_tracking",
    "wofdm_rx_profile_coded", "wofdm_code_steps", "wofdm_viterbi_decode",
    "wofdm_viterbi_decode_long", "wofdm_rx_profile_coded_frame",
    "wofdm_ldpc_lift", "wofdm_ldpc_decode", "wofdm_rx_profile_ldpc",
    "wofdm_coset_info", "wofdm_conv_encode", "wofdm_ldpc_encode", "wofdm_rx_profile_coset",
    "wofdm_ldpc_harq_decode", "wofdm_rx_profile_harq",
)


class WofdmError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "WOFDM_E_?"), code, message))
        self.code = code


class Cfg(C.Structure):
    """Mirror of ``wofdm_cfg``."""
    _fields_ = [(n, C.c_int32) for n in (
        "n_fft", "bits_per_sc", "syms_per_frame", "cp", "cs", "tail_tx", "tail_rx", "prefix_rm",
        "circ_shift", "n_taps", "n_channels", "n_snr", "n_window_pairs",
        "noise_before_truncate")] + [
        ("frames_per_cell", C.c_uint64), ("frame_offset", C.c_uint64), ("seed", C.c_uint64)]

    @property
    def sym_len(self):
        return self.n_fft + self.cp + self.cs

    @property
    def stride(self):
        return self.sym_len - self.tail_tx

    @property
    def frame_len(self):
        return self.tail_tx + self.syms_per_frame * self.stride

    @property
    def n_cells(self):
        return self.n_window_pairs * self.n_snr * self.n_channels


class PsdJob(C.Structure):
    """Mirror of ``wofdm_psd_job``."""
    _fields_ = [(n, C.c_int32) for n in ("block", "cp", "cs", "overlap")]


class SyncPoint(C.Structure):
    """Mirror of ``wofdm_sync_point`` (16 bytes)."""
    _fields_ = [("timing", C.c_int32), ("cfo", C.c_float), ("cfo_tracked", C.c_int32), ("reserved", C.c_int32)]


class PaPoint(C.Structure):
    """Mirror of ``wofdm_pa_point`` (16 bytes)."""
    _fields_ = [("model", C.c_int32), ("ibo_db", C.c_float), ("smooth", C.c_float), ("reserved", C.c_int32)]


class PnPoint(C.Structure):
    """Mirror of ``wofdm_pn_point`` (16 bytes)."""
    _fields_ = [("linewidth", C.c_float), ("cpe_tracked", C.c_int32), ("reserved", C.c_int32 * 2)]


class LinkPoint(C.Structure):
    """Mirror of ``wofdm_link_point`` (64 bytes)."""
    _fields_ = [("pa_model", C.c_int32), ("pa_ibo_db", C.c_float), ("pa_smooth", C.c_float), ("track", C.c_int32),
                ("timing", C.c_int32), ("cfo", C.c_float), ("cfo_tracked", C.c_int32), ("linewidth", C.c_float),
                ("cpe_tracked", C.c_int32), ("aci_on", C.c_int32), ("aci_delay", C.c_int32), ("aci_level_db", C.c_float),
                ("reserved", C.c_int32 * 4)]


class TrackingPoint(C.Structure):
    """Mirror of ``wofdm_tracking_point`` (16 bytes)."""
    _fields_ = [("cpe", C.c_int32), ("post", C.c_int32), ("reserved", C.c_int32 * 2)]


class Code(C.Structure):
    """Mirror of ``wofdm_code`` (16 bytes)."""
    _fields_ = [("rate", C.c_int32), ("reserved", C.c_int32 * 3)]


class LdpcCode(C.Structure):
    """Mirror of ``wofdm_ldpc_code`` (16 bytes)."""
    _fields_ = [("J", C.c_int32), ("L", C.c_int32), ("max_iter", C.c_int32), ("reserved", C.c_int32)]


class Dump(C.Structure):
    """Mirror of ``wofdm_dump`` (host buffers)."""
    _fields_ = [(n, C.c_void_p) for n in ("labels_tx", "X", "tx", "conv", "rx", "Y", "Xhat",
                                          "labels_rx", "gain", "unit_noise")]


def kernel_source_hash():
    """sha256 (first 16 hex digits) over the kernel sources and their build flags: what a committed
    measurement of the kernel (profiles/hbm_traffic.json) is stamped with."""
    import hashlib
    h = hashlib.sha256()
    for name in ("wofdm_kernel.hip", "wofdm_kernel.h", "philox.h", "Makefile"):
        with open(os.path.join(_HERE, "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build(verbose=False):
    """Compile libwofdm_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], check=True, stdout=out)
    return LIB_PATH


def load():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64/libhsa.  If
    # this library pulled in /opt/rocm's copy first, a later `import torch` would find "No HIP
    # GPUs".  Importing torch first (when it is installed) makes both share torch's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `make -C %s` (hipcc, gfx950). The w-OFDM hot path has "
            "no CPU fallback." % (LIB_PATH, os.path.join(_HERE, "csrc")))
    L = C.CDLL(LIB_PATH)
    vp, u64 = C.c_void_p, C.c_uint64
    L.wofdm_version.restype = C.c_int
    L.wofdm_device_count.restype = C.c_int
    L.wofdm_last_error.restype = C.c_char_p
    L.wofdm_noise_len.argtypes = [C.POINTER(Cfg)]
    L.wofdm_plan_create.argtypes = [C.POINTER(vp), C.POINTER(Cfg), C.c_int, vp, vp, vp, vp]
    L.wofdm_plan_destroy.argtypes = [vp]
    L.wofdm_plan_launch.argtypes = [vp, u64, u64, vp, vp]
    L.wofdm_plan_launch_timed.argtypes = [vp, u64, u64, vp, vp, C.POINTER(C.c_float)]
    L.wofdm_plan_launch_injected.argtypes = [vp, u64, vp, vp, vp, vp]
    L.wofdm_plan_dump_frame.argtypes = [vp, C.c_uint32, u64, vp, vp, vp, C.POINTER(Dump)]
    L.wofdm_plan_info.argtypes = [vp, vp]
    L.wofdm_plan_kernel_id.argtypes = [vp, vp]
    L.wofdm_plan_kernel_geo.argtypes = [vp, C.POINTER(C.c_int32)]
    L.wofdm_cfg_geo_id.argtypes = [C.POINTER(Cfg)]
    L.wofdm_plan_set_allocation.argtypes = [vp, vp]
    L.wofdm_plan_set_tx_mask.argtypes = [vp, vp]
    L.wofdm_plan_status.argtypes = [vp]
    L.wofdm_plan_set_option.argtypes = [vp, C.c_int32, C.c_int32]
    L.wofdm_run.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp]
    L.wofdm_run_injected.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_philox_kat.argtypes = [C.c_int, vp, vp, vp]
    L.wofdm_interference.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp]
    L.wofdm_interference_masked.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_tx_psd.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, C.c_int, C.c_int, vp]
    i32 = C.c_int32
    L.wofdm_tx_psd_batch.argtypes = [i32, C.c_int, i32, vp, vp, i32, i32, vp, vp]
    L.wofdm_tx_psd_batch_masked.argtypes = [i32, C.c_int, i32, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp]
    L.wofdm_tx_papr.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, C.c_float, C.c_float, i32, vp, vp, vp]
    L.wofdm_tx_papr_kernel_ms.argtypes = [C.POINTER(C.c_float)]
    L.wofdm_rx_profile.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_rx_profile_aci.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, i32, C.c_float, vp, vp]
    L.wofdm_rx_profile_kernel_ms.argtypes = [C.POINTER(C.c_float)]
    L.wofdm_rx_profile_sync.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, i32, C.POINTER(SyncPoint), vp, vp, vp, vp]
    L.wofdm_rx_profile_doppler.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_rx_profile_pa.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, i32, C.POINTER(PaPoint), vp, vp, vp, vp, vp, vp]
    L.wofdm_rx_profile_pn.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, i32, C.POINTER(PnPoint), vp, vp, vp, vp]
    L.wofdm_rx_profile_link.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                        C.POINTER(LinkPoint), vp, vp, vp, vp, vp]
    L.wofdm_rx_profile_soft.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                        C.POINTER(LinkPoint), i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_rx_profile_tracking.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                            C.POINTER(LinkPoint), i32, vp, vp, C.POINTER(TrackingPoint), vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_rx_profile_coded.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                         C.POINTER(LinkPoint), i32, vp, vp, C.POINTER(TrackingPoint), C.c_float, vp, i32,
                                         C.POINTER(Code), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_code_steps.argtypes = [i32, i32]
    L.wofdm_code_steps.restype = C.c_int
    L.wofdm_viterbi_decode.argtypes = [C.c_int, i32, i32, vp, i32, vp, vp, vp]
    L.wofdm_viterbi_decode_long.argtypes = [C.c_int, i32, i32, vp, i32, vp, vp, vp]
    L.wofdm_rx_profile_coded_frame.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                               C.POINTER(LinkPoint), i32, vp, vp, C.POINTER(TrackingPoint), C.c_float, vp, i32,
                                               C.POINTER(Code), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_ldpc_lift.argtypes = [i32, i32, i32]
    L.wofdm_ldpc_lift.restype = C.c_int
    L.wofdm_ldpc_decode.argtypes = [C.c_int, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp]
    L.wofdm_rx_profile_ldpc.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                        C.POINTER(LinkPoint), i32, vp, vp, C.POINTER(TrackingPoint), C.c_float, vp, i32,
                                        C.POINTER(LdpcCode), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_coset_info.argtypes = [u64, C.c_uint32, u64, i32, vp]
    L.wofdm_conv_encode.argtypes = [C.c_int, i32, i32, i32, vp, vp]
    L.wofdm_ldpc_encode.argtypes = [C.c_int, i32, i32, i32, i32, vp, vp]
    L.wofdm_rx_profile_coset.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                         C.POINTER(LinkPoint), i32, vp, vp, C.POINTER(TrackingPoint), C.c_float, vp, i32,
                                         C.POINTER(Code), i32, C.POINTER(LdpcCode), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_ldpc_harq_decode.argtypes = [C.c_int, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.wofdm_rx_profile_harq.argtypes = [C.POINTER(Cfg), C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, i32,
                                        C.POINTER(LinkPoint), i32, vp, vp, C.POINTER(TrackingPoint), C.c_float, vp, i32,
                                        C.POINTER(LdpcCode), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.wofdm_tx_psd_batch_pa.argtypes = [i32, C.c_int, i32, vp, vp, i32, vp, vp, vp, i32, C.POINTER(PaPoint), vp, i32, i32, vp, vp, vp]
    _LIB = L
    return L


def check(rc):
    if rc != WOFDM_OK:
        raise WofdmError(rc, load().wofdm_last_error().decode("utf-8", "replace"))
    return rc


def f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), a.shape))
    return a


def c64_as_f32(a, shape=None):
    """complex array -> contiguous float32 array with a trailing (re, im) axis"""
    a = np.ascontiguousarray(a, dtype=np.complex64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), a.shape))
    return a.view(np.float32).reshape(a.shape + (2,))
