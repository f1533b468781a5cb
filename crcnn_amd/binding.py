"""ctypes binding of libcrcnn_hip.so (the C ABI in include/crcnn_hip.h).

This module is plumbing: it loads the in-tree shared library, checks that every symbol the header declares is
exported, and offers a small `Engine` convenience class (device buffers + numpy round trips) for tests, the bench
harness and Python users.  There is NO CPU fallback: a missing library or a failing call raises.
"""
import ctypes
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcrcnn_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "crcnn_hip.h")

u64 = ctypes.c_uint64
PU = ctypes.POINTER(u64)
VP = ctypes.c_void_p
CI = ctypes.c_int
SZ = ctypes.c_size_t

COEFF, NTT, NTTP, NTTL, NTTL1, NTTLC, NTTLS = 0, 1, 2, 3, 4, 5, 6


class CrcError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        super().__init__(f"{what}: {_strerror(status)} (status {status}, hip error {_lib.crc_last_hip_error() if _lib else '?'})")


_lib = None


def header_symbols():
    """names of every function declared in include/crcnn_hip.h"""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(crc_[a-z0-9_]+)\s*\(", txt)))


def _strerror(s):
    return _lib.crc_strerror(s).decode() if _lib else "?"


def load():
    """dlopen the in-tree library; raises if it was not built (run `python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: the HIP extension has not been built (no CPU fallback exists)")
    try:
        # torch ships its own libamdhip64: load it first so that this library binds to the same HIP runtime (two runtimes in one
        # process cannot both own the device: whichever initialises second sees "no HIP GPUs")
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    missing = [s for s in header_symbols() if not hasattr(L, s)]
    if missing:
        raise ImportError(f"libcrcnn_hip.so does not export: {missing}")
    L.crc_strerror.restype = ctypes.c_char_p
    L.crc_strerror.argtypes = [CI]
    L.crc_ctx_create.argtypes = [CI, PU, CI, u64, CI, ctypes.POINTER(VP)]
    L.crc_ctx_destroy.argtypes = [VP]
    L.crc_ctx_destroy.restype = None
    L.crc_default_coeff_modulus_128.argtypes = [CI, PU, CI]
    for f in ("crc_ctx_n", "crc_ctx_k", "crc_ctx_kbsk", "crc_ctx_device"):
        getattr(L, f).argtypes = [VP]
    L.crc_ct_words.restype = SZ; L.crc_ct_words.argtypes = [VP, CI]
    L.crc_evk_words.restype = SZ; L.crc_evk_words.argtypes = [VP, CI]
    L.crc_ctx_table.argtypes = [VP, ctypes.c_char_p, PU, CI]
    L.crc_ctx_set_tuning.argtypes = [VP, ctypes.c_char_p, ctypes.c_longlong]
    L.crc_mem_info.argtypes = [VP, ctypes.POINTER(SZ), ctypes.POINTER(SZ)]
    L.crc_malloc.argtypes = [VP, SZ, ctypes.POINTER(VP)]
    L.crc_free.argtypes = [VP, VP]
    L.crc_memcpy_h2d.argtypes = [VP, VP, VP, SZ, VP]
    L.crc_memcpy_d2h.argtypes = [VP, VP, VP, SZ, VP]
    L.crc_memcpy_d2d.argtypes = [VP, VP, VP, SZ, VP]
    L.crc_memset.argtypes = [VP, VP, CI, SZ, VP]
    L.crc_stream_sync.argtypes = [VP, VP]
    L.crc_event_create.argtypes = [VP, ctypes.POINTER(VP)]; L.crc_event_destroy.argtypes = [VP, VP]; L.crc_event_record.argtypes = [VP, VP, VP]
    L.crc_event_elapsed_ms.argtypes = [VP, VP, VP, ctypes.POINTER(ctypes.c_float)]
    L.crc_stream_create.argtypes = [VP, ctypes.POINTER(VP)]; L.crc_stream_destroy.argtypes = [VP, VP]; L.crc_stream_wait_event.argtypes = [VP, VP, VP]
    L.crc_host_alloc.argtypes = [VP, SZ, ctypes.POINTER(VP)]; L.crc_host_free.argtypes = [VP, VP]
    L.crc_host_thread_limit.argtypes = []
    L.crc_encode_f32.argtypes = [VP, ctypes.POINTER(ctypes.c_float), SZ, PU, ctypes.POINTER(ctypes.c_int32)]
    L.crc_encode_f64.argtypes = [VP, ctypes.POINTER(ctypes.c_double), SZ, PU, ctypes.POINTER(ctypes.c_int32)]
    L.crc_decode.restype = ctypes.c_double; L.crc_decode.argtypes = [VP, PU]
    L.crc_bn_invstd_f32.argtypes = [ctypes.POINTER(ctypes.c_float), SZ, ctypes.POINTER(ctypes.c_float)]
    L.crc_plain_to_ntt.argtypes = [VP, VP, SZ, VP, VP]
    L.crc_encode_f32_compact.argtypes = [VP, ctypes.POINTER(ctypes.c_float), SZ, PU, ctypes.POINTER(ctypes.c_int32)]
    L.crc_plain_expand.argtypes = [VP, VP, SZ, VP, VP]
    L.crc_plain_to_delta.argtypes = [VP, VP, SZ, CI, VP, VP]
    L.crc_ntt_fwd.argtypes = [VP, VP, SZ, CI, VP]
    L.crc_ntt_inv.argtypes = [VP, VP, SZ, CI, VP]
    L.crc_ntt_fwd_box.argtypes = [VP, VP, VP] + [CI] * 7 + [VP]
    L.crc_ntt_fwd_bsk.argtypes = [VP, VP, SZ, VP]
    L.crc_ntt_inv_bsk.argtypes = [VP, VP, SZ, VP]
    L.crc_add.argtypes = [VP, VP, VP, SZ, CI, VP]
    L.crc_add_plain.argtypes = [VP, VP, VP, SZ, SZ, CI, VP]
    L.crc_multiply_plain_ntt.argtypes = [VP, VP, VP, SZ, SZ, CI, VP]
    L.crc_multiply_plain.argtypes = [VP, VP, VP, SZ, SZ, VP]
    L.crc_conv2d_work_bytes.restype = SZ; L.crc_conv2d_work_bytes.argtypes = [VP] + [CI] * 10
    L.crc_conv2d.argtypes = [VP, VP, VP, VP] + [CI] * 11 + [VP, VP, VP]
    L.crc_conv2d_fold_pool.argtypes = [VP, VP, VP, VP] + [CI] * 8 + [VP, VP, VP]
    L.crc_conv2d_hoist_pool.argtypes = [VP, VP, VP, VP] + [CI] * 6 + [VP, VP, VP]
    L.crc_dense_work_bytes.restype = SZ; L.crc_dense_work_bytes.argtypes = [VP, CI, CI, CI, CI]
    L.crc_dense.argtypes = [VP, VP, VP, VP, CI, CI, CI, CI, CI, VP, VP, VP]
    L.crc_pool.argtypes = [VP, VP] + [CI] * 8 + [VP, CI, VP, VP]
    L.crc_batchnorm.argtypes = [VP, VP, CI, CI, CI, CI, VP, VP, CI, VP]
    L.crc_pad.argtypes = [VP, VP] + [CI] * 9 + [VP, VP]
    L.crc_square_relin_work_bytes.restype = SZ; L.crc_square_relin_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_square_relin.argtypes = [VP, VP, SZ, VP, CI, VP, VP, VP]
    L.crc_square_relin_forms.argtypes = [VP, VP, CI, SZ, VP, CI, VP, CI, VP, VP]
    L.crc_square_pool_relin_supported.argtypes = [VP, CI, CI, CI]
    L.crc_square_pool_relin_work_bytes.restype = SZ; L.crc_square_pool_relin_work_bytes.argtypes = [VP] + [CI] * 9
    L.crc_square_pool_relin_forms.argtypes = [VP, VP, CI] + [CI] * 8 + [VP, CI, VP, VP, CI, VP, VP]
    L.crc_poly2_relin_work_bytes.restype = SZ; L.crc_poly2_relin_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_poly2_relin_forms.argtypes = [VP, VP, CI, SZ, VP, CI, VP, VP, VP, VP, CI, VP, VP]
    L.crc_multiply_relin_work_bytes.restype = SZ; L.crc_multiply_relin_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_multiply.argtypes = [VP, VP, VP, SZ, VP, VP, VP]
    L.crc_multiply_relin_forms.argtypes = [VP, VP, VP, CI, SZ, VP, CI, VP, CI, VP, VP]
    L.crc_poly3_relin_work_bytes.restype = SZ; L.crc_poly3_relin_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_poly3_relin_forms.argtypes = [VP, VP, CI, SZ, VP, CI, VP, VP, VP, VP, VP, CI, VP, VP]
    L.crc_poly2_pool_relin_supported.argtypes = [VP, CI, CI, CI]
    L.crc_poly2_pool_relin_work_bytes.restype = SZ; L.crc_poly2_pool_relin_work_bytes.argtypes = [VP] + [CI] * 9
    L.crc_poly2_pool_relin_forms.argtypes = [VP, VP, CI] + [CI] * 8 + [VP, CI, VP, VP, VP, VP, CI, VP, VP]
    L.crc_conv2d_forms.argtypes = [VP, VP, VP, CI, VP] + [CI] * 9 + [CI, CI, VP, VP, VP]
    L.crc_dense_forms.argtypes = [VP, VP, VP, CI, VP, CI, CI, CI, CI, CI, VP, VP, VP]
    L.crc_pack28.argtypes = [VP, VP, SZ, CI, VP]
    L.crc_limb_supported.argtypes = [VP, CI, CI, CI]
    L.crc_limb_tensor_bytes.restype = SZ; L.crc_limb_tensor_bytes.argtypes = [VP, CI, CI, CI, CI]
    L.crc_limb_weights_bytes.restype = SZ; L.crc_limb_weights_bytes.argtypes = [VP, CI, CI, CI, CI]
    L.crc_limb_pack_weights.argtypes = [VP, VP, CI, CI, CI, CI, VP, VP]
    L.crc_limb_pack_weights_tile.argtypes = [VP, VP, CI, CI, CI, CI, CI, CI, VP, VP]
    L.crc_limb_pack_tensor_at.argtypes = [VP, VP, CI, CI, CI, CI, CI, VP, CI, CI, VP]
    L.crc_plan_mac.argtypes = [VP] + [CI] * 10 + [ctypes.POINTER(CI)]
    L.crc_plan_mac_scalar.argtypes = [VP] + [CI] * 9 + [ctypes.POINTER(CI)]
    L.crc_scalar_weights_bytes.restype = SZ; L.crc_scalar_weights_bytes.argtypes = [VP, CI, CI, CI, CI]
    L.crc_scalar_supported.argtypes = [VP] + [CI] * 9
    L.crc_scalar_pack_weights.argtypes = [VP, VP, CI, CI, CI, CI, CI, VP, ctypes.POINTER(CI), VP]
    L.crc_plan_fold_pool.argtypes = [VP] + [CI] * 12 + [ctypes.POINTER(CI)]
    L.crc_plan_hoist_pool.argtypes = [VP] + [CI] * 22 + [ctypes.POINTER(CI)]
    L.crc_limb_pack_tensor.argtypes = [VP, VP, CI, CI, CI, CI, CI, VP, VP]
    L.crc_limb_conv1_supported.argtypes = [VP] + [CI] * 8
    L.crc_limb_conv1_box_supported.argtypes = [VP] + [CI] * 10
    L.crc_conv2d_box_forms_work_bytes.restype = SZ; L.crc_conv2d_box_forms_work_bytes.argtypes = [VP] + [CI] * 14
    L.crc_conv2d_box_forms.argtypes = [VP, VP, VP, CI, VP] + [CI] * 11 + [CI, CI, VP, VP, VP]
    L.crc_plan_conv1_box.argtypes = [VP] + [CI] * 12 + [ctypes.POINTER(CI)]
    L.crc_limb_conv1_weights_bytes.restype = SZ; L.crc_limb_conv1_weights_bytes.argtypes = [VP]
    L.crc_limb_conv1_pack_weights.argtypes = [VP, VP, CI, CI, CI, VP, VP]
    L.crc_limb_conv1_weights_bytes_for.restype = SZ; L.crc_limb_conv1_weights_bytes_for.argtypes = [VP, CI, CI, CI]
    L.crc_limb_conv1_form.argtypes = [VP] + [CI] * 8
    L.crc_conv2d_forms_work_bytes.restype = SZ; L.crc_conv2d_forms_work_bytes.argtypes = [VP] + [CI] * 12
    L.crc_square.argtypes = [VP, VP, SZ, VP, VP, VP]
    L.crc_relinearize.argtypes = [VP, VP, SZ, VP, CI, VP, VP, VP]
    L.crc_import_seal.argtypes = [VP, PU, CI, PU]
    L.crc_export_seal.argtypes = [VP, PU, CI, PU]
    L.crc_params_hash.argtypes = [VP, PU]
    for f_ in ("ct", "evk", "pk", "sk"):
        getattr(L, f"crc_seal_{f_}_bytes").restype = SZ
    L.crc_seal_ct_bytes.argtypes = [VP, CI]; L.crc_seal_evk_bytes.argtypes = [VP, CI]; L.crc_seal_pk_bytes.argtypes = [VP]; L.crc_seal_sk_bytes.argtypes = [VP]
    L.crc_seal_ct_save.argtypes = [VP, PU, CI, VP, SZ, ctypes.POINTER(SZ)]
    L.crc_seal_ct_load.argtypes = [VP, VP, SZ, PU, CI, ctypes.POINTER(CI), ctypes.POINTER(SZ)]
    L.crc_seal_evk_save.argtypes = [VP, PU, CI, VP, SZ, ctypes.POINTER(SZ)]
    L.crc_seal_evk_load.argtypes = [VP, VP, SZ, PU, ctypes.POINTER(CI)]
    L.crc_seal_pk_save.argtypes = [VP, PU, VP, SZ, ctypes.POINTER(SZ)]
    L.crc_seal_pk_load.argtypes = [VP, VP, SZ, PU]
    L.crc_seal_sk_save.argtypes = [VP, PU, VP, SZ, ctypes.POINTER(SZ)]
    L.crc_seal_sk_load.argtypes = [VP, VP, SZ, PU]
    L.crc_h5_dataset_count.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(SZ)]
    L.crc_h5_read_f32.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_float), SZ, ctypes.POINTER(SZ)]
    L.crc_h5_list.argtypes = [ctypes.c_char_p, ctypes.c_char_p, SZ]
    L.crc_keygen.argtypes = [VP, u64, PU, PU]
    L.crc_gen_evk.argtypes = [VP, u64, PU, CI, PU]
    L.crc_encrypt.argtypes = [VP, PU, PU, SZ, u64, PU]
    L.crc_encrypt_dev_work_bytes.restype = SZ; L.crc_encrypt_dev_work_bytes.argtypes = [VP, SZ]
    L.crc_encrypt_dev.argtypes = [VP, VP, VP, SZ, u64, VP, VP, VP]
    PB = ctypes.POINTER(ctypes.c_uint8)
    L.crc_random_key.argtypes = [PB]
    L.crc_chacha20_block.argtypes = [PB, ctypes.c_uint32, PB, PB]
    L.crc_keygen_key.argtypes = [VP, PB, PU, PU]
    L.crc_gen_evk_key.argtypes = [VP, PB, PU, CI, PU]
    L.crc_encrypt_key.argtypes = [VP, PU, PU, SZ, PB, u64, PU]
    L.crc_encrypt_dev_key.argtypes = [VP, VP, VP, SZ, PB, u64, VP, VP, VP]
    L.crc_encrypt_dev_forms.argtypes = [VP, VP, VP, SZ, u64, ctypes.c_int, VP, VP, VP]
    L.crc_encrypt_dev_key_forms.argtypes = [VP, VP, VP, SZ, PB, u64, ctypes.c_int, VP, VP, VP]
    L.crc_encrypt_dev_noise_thresholds.restype = None; L.crc_encrypt_dev_noise_thresholds.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    L.crc_decrypt_dev_work_bytes.restype = SZ; L.crc_decrypt_dev_work_bytes.argtypes = [VP, SZ, CI, CI]
    L.crc_decrypt_dev.argtypes = [VP, VP, VP, SZ, CI, CI, VP, VP, VP]
    L.crc_noise_budget_dev_work_bytes.restype = SZ; L.crc_noise_budget_dev_work_bytes.argtypes = [VP, SZ, CI, CI]
    L.crc_noise_budget_dev.argtypes = [VP, VP, VP, SZ, CI, CI, VP, VP, VP, VP]
    L.crc_budget_bits_host.argtypes = [VP, PU, SZ, ctypes.POINTER(ctypes.c_int32)]
    L.crc_decode_dev.argtypes = [VP, VP, SZ, VP, VP]
    L.crc_slots_supported.argtypes = [VP]
    L.crc_slots_prime.argtypes = [CI, CI, PU]
    PI64 = ctypes.POINTER(ctypes.c_int64)
    L.crc_slots_compose.argtypes = [VP, PI64, SZ, CI, SZ, SZ, PU]
    L.crc_slots_decompose.argtypes = [VP, PU, SZ, CI, PI64, SZ, SZ]
    L.crc_slots_compose_dev.argtypes = [VP, VP, SZ, CI, SZ, SZ, VP, VP]
    L.crc_slots_decompose_dev.argtypes = [VP, VP, SZ, CI, VP, SZ, SZ, VP]
    L.crc_slots_rescale.argtypes = [VP, PU, SZ, u64, PU]
    L.crc_slots_rescale_dev.argtypes = [VP, VP, SZ, u64, VP, VP]
    L.crc_slots_refresh_dev_work_bytes.restype = SZ; L.crc_slots_refresh_dev_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_slots_refresh_dev.argtypes = [VP, VP, VP, VP, SZ, CI, u64, u64, CI, VP, VP, VP]
    L.crc_slots_refresh_dev_key.argtypes = [VP, VP, VP, VP, SZ, CI, u64, PB, u64, CI, VP, VP, VP]
    L.crc_slots_refresh_sym_dev_work_bytes.restype = SZ; L.crc_slots_refresh_sym_dev_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_slots_refresh_sym_dev.argtypes = [VP, VP, VP, SZ, CI, u64, u64, CI, VP, VP, VP]
    L.crc_slots_refresh_sym_dev_key.argtypes = [VP, VP, VP, SZ, CI, u64, PB, u64, CI, VP, VP, VP]
    WIN = [CI] * 6                                             # xd, yd, xs, ys, xf, yf
    L.crc_slots_act.argtypes = [VP, PU, SZ] + WIN + [u64, CI, u64, PU]
    L.crc_slots_act_dev.argtypes = [VP, VP, SZ] + WIN + [u64, CI, u64, VP, VP]
    L.crc_slots_refresh_act_dev_work_bytes.restype = SZ; L.crc_slots_refresh_act_dev_work_bytes.argtypes = [VP, SZ] + WIN + [CI]
    L.crc_slots_refresh_act_dev.argtypes = [VP, VP, VP, VP, SZ] + WIN + [CI, u64, CI, u64, u64, CI, VP, VP, VP]
    L.crc_slots_refresh_act_dev_key.argtypes = [VP, VP, VP, VP, SZ] + WIN + [CI, u64, CI, u64, PB, u64, CI, VP, VP, VP]
    L.crc_slots_refresh_act_sym_dev_work_bytes.restype = SZ; L.crc_slots_refresh_act_sym_dev_work_bytes.argtypes = [VP, SZ] + WIN + [CI]
    L.crc_slots_refresh_act_sym_dev.argtypes = [VP, VP, VP, SZ] + WIN + [CI, u64, CI, u64, u64, CI, VP, VP, VP]
    L.crc_slots_refresh_act_sym_dev_key.argtypes = [VP, VP, VP, SZ] + WIN + [CI, u64, CI, u64, PB, u64, CI, VP, VP, VP]
    PVP = ctypes.POINTER(VP)                                   # a host array of r contexts / row pointers
    L.crc_slots_crt_supported.argtypes = [PVP, CI]
    L.crc_slots_crt_primes.argtypes = [CI, CI, CI, PU]
    L.crc_slots_crt_decompose.argtypes = [PVP, CI, PVP, SZ, CI, PI64, SZ, SZ]
    L.crc_slots_crt_decompose_dev.argtypes = [PVP, CI, PVP, SZ, CI, VP, SZ, SZ, VP]
    L.crc_slots_crt_act.argtypes = [PVP, CI, PVP, SZ, u64, CI, u64, PVP]
    L.crc_slots_crt_act_dev.argtypes = [PVP, CI, PVP, SZ, u64, CI, u64, PVP, VP]
    L.crc_slots_crt_refresh_dev_work_bytes.restype = SZ; L.crc_slots_crt_refresh_dev_work_bytes.argtypes = [PVP, CI, SZ, CI]
    L.crc_slots_crt_refresh_dev_key.argtypes = [PVP, CI, VP, VP, PVP, SZ, CI, u64, CI, u64, PB, u64, CI, PVP, VP, VP]
    L.crc_slots_crt_refresh_sym_dev_key.argtypes = [PVP, CI, VP, PVP, SZ, CI, u64, CI, u64, PB, u64, CI, PVP, VP, VP]
    L.crc_encode_dev_f32.argtypes = [VP, VP, SZ, VP, VP]
    L.crc_encode_dev_f64.argtypes = [VP, VP, SZ, VP, VP]
    L.crc_refresh_dev_work_bytes.restype = SZ; L.crc_refresh_dev_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_refresh_dev.argtypes = [VP, VP, VP, VP, SZ, CI, u64, CI, VP, VP, VP, VP]
    L.crc_refresh_dev_key.argtypes = [VP, VP, VP, VP, SZ, CI, PB, u64, CI, VP, VP, VP, VP]
    L.crc_encrypt_sym.argtypes = [VP, PU, PU, SZ, u64, CI, PU]
    L.crc_encrypt_sym_key.argtypes = [VP, PU, PU, SZ, PB, u64, CI, PU]
    L.crc_encrypt_sym_dev_work_bytes.restype = SZ; L.crc_encrypt_sym_dev_work_bytes.argtypes = [VP, SZ]
    L.crc_encrypt_sym_dev_forms.argtypes = [VP, VP, VP, SZ, u64, CI, VP, VP, VP]
    L.crc_encrypt_sym_dev_key_forms.argtypes = [VP, VP, VP, SZ, PB, u64, CI, VP, VP, VP]
    L.crc_refresh_sym_dev_work_bytes.restype = SZ; L.crc_refresh_sym_dev_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_refresh_sym_dev.argtypes = [VP, VP, VP, SZ, CI, u64, CI, VP, VP, VP, VP]
    L.crc_refresh_sym_dev_key.argtypes = [VP, VP, VP, SZ, CI, PB, u64, CI, VP, VP, VP, VP]
    L.crc_seeded_public_seed.argtypes = [u64, PB]
    L.crc_encrypt_sym_seeded.argtypes = [VP, PU, PU, SZ, u64, PU]
    L.crc_encrypt_sym_seeded_key.argtypes = [VP, PU, PU, SZ, PB, PB, u64, PU]
    L.crc_seeded_expand.argtypes = [VP, PU, SZ, PB, u64, CI, PU]
    L.crc_seeded_expand_dev.argtypes = [VP, VP, SZ, PB, u64, CI, VP, VP]
    L.crc_encrypt_sym_seeded_dev.argtypes = [VP, VP, VP, SZ, u64, VP, VP]
    L.crc_encrypt_sym_seeded_dev_key.argtypes = [VP, VP, VP, SZ, PB, PB, u64, VP, VP]
    L.crc_encrypt_f32_seeded_dev_work_bytes.restype = SZ; L.crc_encrypt_f32_seeded_dev_work_bytes.argtypes = [VP, SZ]
    L.crc_encrypt_f32_seeded_dev.argtypes = [VP, VP, VP, SZ, u64, VP, VP, VP]
    L.crc_encrypt_f32_seeded_dev_key.argtypes = [VP, VP, VP, SZ, PB, PB, u64, VP, VP, VP]
    L.crc_seeded_ct_bytes.restype = SZ; L.crc_seeded_ct_bytes.argtypes = [VP, SZ]
    L.crc_seeded_ct_save.argtypes = [VP, PU, SZ, PB, u64, VP, SZ, ctypes.POINTER(SZ)]
    L.crc_seeded_ct_load.argtypes = [VP, VP, SZ, PU, SZ, ctypes.POINTER(SZ), PB, ctypes.POINTER(u64)]
    L.crc_seeded_key_words.restype = SZ; L.crc_seeded_key_words.argtypes = [VP, CI]
    L.crc_gen_keys_seeded.argtypes = [VP, u64, PU, CI, PU, CI, PU]
    L.crc_gen_keys_seeded_key.argtypes = [VP, PB, PB, PU, CI, PU, CI, PU]
    L.crc_seeded_keys_expand.argtypes = [VP, PU, PU, CI, CI, PB, CI, PU]
    L.crc_gen_keys_seeded_dev.argtypes = [VP, u64, VP, CI, PU, CI, VP, VP]
    L.crc_gen_keys_seeded_dev_key.argtypes = [VP, PB, PB, VP, CI, PU, CI, VP, VP]
    L.crc_seeded_keys_expand_dev.argtypes = [VP, VP, PU, CI, CI, PB, CI, VP, VP]
    L.crc_seeded_keys_bytes.restype = SZ; L.crc_seeded_keys_bytes.argtypes = [VP, CI, CI]
    L.crc_seeded_keys_save.argtypes = [VP, PU, PU, CI, CI, PB, VP, SZ, ctypes.POINTER(SZ)]
    L.crc_seeded_keys_load.argtypes = [VP, VP, SZ, PU, PU, CI, ctypes.POINTER(CI), ctypes.POINTER(CI), PB]
    L.crc_comm_unique_id.argtypes = [PB]
    L.crc_comm_create.argtypes = [VP, CI, CI, PB, ctypes.POINTER(VP)]
    L.crc_comm_create_all.argtypes = [ctypes.POINTER(VP), CI, ctypes.POINTER(VP)]
    L.crc_comm_destroy.argtypes = [VP]; L.crc_comm_destroy.restype = None
    L.crc_comm_rank.argtypes = [VP]; L.crc_comm_world.argtypes = [VP]
    L.crc_broadcast_weights.argtypes = [VP, VP, SZ, CI, VP]
    L.crc_broadcast_weights_all.argtypes = [ctypes.POINTER(VP), CI, ctypes.POINTER(VP), SZ, CI, ctypes.POINTER(VP)]
    L.crc_comm_allgather_u64.argtypes = [VP, PU, SZ, PU, VP]
    L.crc_checksum64.argtypes = [VP, VP, SZ, PU, VP]
    L.crc_decrypt.argtypes = [VP, PU, PU, SZ, CI, PU]
    PI = ctypes.POINTER(CI)
    L.crc_galois_elt_valid.argtypes = [VP, u64]
    L.crc_galois_elt_rows.restype = u64; L.crc_galois_elt_rows.argtypes = [VP, CI]
    L.crc_galois_elt_columns.restype = u64; L.crc_galois_elt_columns.argtypes = [VP]
    L.crc_galois_default_elts.argtypes = [VP, PU, CI]
    L.crc_gen_galois_keys.argtypes = [VP, u64, PU, CI, PU, CI, PU]
    L.crc_gen_galois_keys_key.argtypes = [VP, PB, PU, CI, PU, CI, PU]
    L.crc_galois_plan.argtypes = [VP, u64, PU, CI, PI, CI]
    L.crc_galois_permute_dev.argtypes = [VP, VP, SZ, u64, CI, VP, VP]
    L.crc_apply_galois_work_bytes.restype = SZ; L.crc_apply_galois_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_apply_galois_forms.argtypes = [VP, VP, CI, SZ, u64, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_rotate_rows_forms.argtypes = [VP, VP, CI, SZ, CI, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_rotate_columns_forms.argtypes = [VP, VP, CI, SZ, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_sum_slots_work_bytes.restype = SZ; L.crc_sum_slots_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_sum_slots_forms.argtypes = [VP, VP, CI, SZ, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_galois_ntt_table.argtypes = [VP, u64, ctypes.POINTER(ctypes.c_uint32)]
    L.crc_galois_conjugate_keys.argtypes = [VP, PU, CI, CI, PU, PU]
    L.crc_galois_conjugate_keys_dev.argtypes = [VP, PU, CI, CI, VP, VP, VP]
    L.crc_galois_permute_ntt_dev.argtypes = [VP, VP, SZ, u64, VP, VP]
    L.crc_rotate_hoisted_work_bytes.restype = SZ; L.crc_rotate_hoisted_work_bytes.argtypes = [VP, SZ, CI, CI]
    L.crc_rotate_hoisted_forms.argtypes = [VP, VP, CI, SZ, PU, CI, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_diag_mac_work_bytes.restype = SZ; L.crc_diag_mac_work_bytes.argtypes = [VP, SZ, CI, CI]
    L.crc_diag_mac_forms.argtypes = [VP, VP, CI, SZ, PU, CI, VP, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_diag_mac_bsgs_work_bytes.restype = SZ; L.crc_diag_mac_bsgs_work_bytes.argtypes = [VP, SZ, CI, CI, CI]
    L.crc_diag_mac_bsgs_forms.argtypes = [VP, VP, CI, SZ, PU, CI, PU, CI, VP, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_conv_slots_pack_weights.argtypes = [VP, ctypes.POINTER(ctypes.c_int64), SZ, PU]
    L.crc_conv_slots_work_bytes.restype = SZ; L.crc_conv_slots_work_bytes.argtypes = [VP, SZ, CI, CI, CI, CI]
    L.crc_conv_slots_forms.argtypes = [VP, VP, CI, SZ, CI, PU, CI, VP, CI, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_conv_slots_pack_bias.argtypes = [VP, ctypes.POINTER(ctypes.c_int64), SZ, PU]
    L.crc_conv_slots_bias_mask_forms.argtypes = [VP, VP, CI, SZ, CI, PU, CI, VP, CI, VP, VP, VP, PU, CI, CI, VP, CI, VP, VP]
    L.crc_galois_prepared_key_words.restype = SZ; L.crc_galois_prepared_key_words.argtypes = [VP, CI]
    L.crc_galois_prepare_keys_dev.argtypes = [VP, VP, PU, CI, CI, VP, VP, VP]
    L.crc_dense_planes_work_bytes.restype = SZ; L.crc_dense_planes_work_bytes.argtypes = [VP, SZ, CI, CI, CI, CI]
    L.crc_dense_planes_forms.argtypes = [VP, VP, CI, SZ, CI, PU, CI, VP, VP, PU, CI, VP, CI, VP, CI, VP, VP]
    L.crc_noise_budget.argtypes = [VP, PU, PU, CI]
    L.crc_mod_switch_supported.argtypes = [VP, VP]
    L.crc_mod_switch_work_bytes.restype = SZ; L.crc_mod_switch_work_bytes.argtypes = [VP, VP, SZ, CI, CI, CI]
    L.crc_mod_switch_forms.argtypes = [VP, VP, VP, CI, SZ, CI, VP, CI, VP, VP]
    L.crc_mod_switch.argtypes = [VP, VP, PU, CI, SZ, CI, PU, CI]
    L.crc_flood_supported.argtypes = [VP, CI]
    L.crc_flood_bits.argtypes = [VP, CI, CI]
    L.crc_flood_budget_bound.argtypes = [VP, CI, CI]
    L.crc_flood_dev_work_bytes.restype = SZ; L.crc_flood_dev_work_bytes.argtypes = [VP, SZ, CI]
    L.crc_flood_dev_key.argtypes = [VP, VP, VP, SZ, CI, CI, PB, u64, VP, VP]
    L.crc_flood_dev.argtypes = [VP, VP, VP, SZ, CI, CI, u64, VP, VP]
    L.crc_flood_key.argtypes = [VP, PU, PU, SZ, CI, CI, PB, u64]
    L.crc_flood.argtypes = [VP, PU, PU, SZ, CI, CI, u64]
    L.crc_ctx_create_level.argtypes = [VP, CI, CI, ctypes.POINTER(VP)]
    L.crc_ctx_key_moduli.argtypes = [VP]
    L.crc_keys_restrict_supported.argtypes = [VP, VP]
    L.crc_keys_restrict.argtypes = [VP, VP, PU, CI, CI, PU]
    L.crc_keys_restrict_dev.argtypes = [VP, VP, VP, CI, CI, VP, VP]
    L.crc_seeded_keys_expand_level.argtypes = [VP, VP, PU, PU, CI, CI, PB, CI, PU]
    L.crc_seeded_keys_expand_level_dev.argtypes = [VP, VP, VP, PU, CI, CI, PB, CI, VP, VP]
    _lib = L
    return L


def _chk(status, what):
    if status < 0:
        raise CrcError(status, what)
    return status


def _pu(a):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(PU)


def default_coeff_modulus_128(n):
    L = load()
    buf = (u64 * 16)()
    cnt = _chk(L.crc_default_coeff_modulus_128(n, buf, 16), "crc_default_coeff_modulus_128")
    return [int(buf[i]) for i in range(cnt)]


def diag_matvec_plan(W, M, n):
    """The diagonal method for y = W x mod t over the slots of one ciphertext.  W: integers (out x in, already reduced mod t, out and in <= M), zero-padded here to
    M x M; M a power of two <= n/2.  Returns (steps, rows): the steps d of the non-zero diagonals and their slot rows [len(steps)][n] (int64),
    rows[r][i] = W[i mod M][(i mod M + d) mod M] -- period M over both rows of n/2 slots.  With x tiled with period M as well, a row rotation by d is a rotation
    mod M, and  y = Sum_r rows[r] (.) rotate_rows(x, steps[r])  holds W x in slots 0..out-1 of every period."""
    W = np.asarray(W)
    if W.ndim != 2 or M < 1 or M & (M - 1) or M > n // 2 or W.shape[0] > M or W.shape[1] > M:
        raise ValueError("diag_matvec_plan: W must be out x in with out, in <= M, M a power of two <= n/2")
    P = np.zeros((M, M), dtype=np.int64)
    P[:W.shape[0], :W.shape[1]] = W
    i = np.arange(M)
    steps, rows = [], []
    for d in range(M):
        diag = P[i, (i + d) % M]
        if diag.any():
            steps.append(d)
            rows.append(np.tile(diag, n // M))
    return steps, np.array(rows, dtype=np.int64).reshape(len(steps), n)


def _bsgs_args(M, n, B, what):
    if M < 1 or M & (M - 1) or M > n // 2 or B < 1 or B & (B - 1) or B > M:
        raise ValueError(what + ": M a power of two <= n/2, B a power of two with 1 <= B <= M")


def bsgs_matvec_plan(W, M, n, B):
    """The baby-step / giant-step form of diag_matvec_plan: the diagonal d = B j + b is reached as a giant rotation by B j of a product with a baby rotation by b,
        y = Sum_j rotate_rows( Sum_b rows[j][b] (.) rotate_rows(x, b), B j ),   rows[j][b][i] = W[(i - B j) mod M][(i + b) mod M]
    (period M over both rows of n/2 slots).  B: a power of two, 1 <= B <= M.  Returns (baby_steps, giant_steps, rows [giant][baby][n] int64): the giant steps B j
    whose group has a non-zero entry, the baby steps b with a non-zero entry in a kept group, zero rows where a pair is empty.  B = M is diag_matvec_plan."""
    W = np.asarray(W)
    _bsgs_args(M, n, B, "bsgs_matvec_plan")
    if W.ndim != 2 or W.shape[0] > M or W.shape[1] > M:
        raise ValueError("bsgs_matvec_plan: W must be out x in with out, in <= M")
    P = np.zeros((M, M), dtype=np.int64)
    P[:W.shape[0], :W.shape[1]] = W
    i = np.arange(M)
    used = np.array([P[i, (i + d) % M].any() for d in range(M)]).reshape(M // B, B)
    giant = [B * j for j in range(M // B) if used[j].any()]
    baby = [b for b in range(B) if used[:, b].any()]
    rows = np.zeros((len(giant), len(baby), n), dtype=np.int64)
    for a, gs in enumerate(giant):
        for c, b in enumerate(baby):
            rows[a, c] = np.tile(P[(i - gs) % M, (i + b) % M], n // M)
    return baby, giant, rows


def bsgs_elements(M, B, n):
    """the Galois elements (3^s mod 2n) a dense M x M product split at B needs: the baby steps 1 .. B - 1, then the giant steps B, 2 B, .. M - B -- what to hand
    to gen_galois_keys"""
    _bsgs_args(M, n, B, "bsgs_elements")
    return [pow(3, s, 2 * n) for s in range(1, M) if s < B or s % B == 0]


class ConvSlotsPlan:
    """What conv_slots_plan returns.  steps [T]: the row rotation of every tap of the (fh + pool - 1) x (fw + pool - 1) window, row-major; elements [T]:
    3^step mod 2n (crc_galois_elt_rows; the tap (0, 0) is the element 1, which needs no key); out_h, out_w, out_dil: the geometry of the valid outputs, output
    (y, x) at slot out_dil (y pitch + x) of every period M; valid: those slots of the first period, row-major.  fold(w, t): the weights the taps take"""
    def __init__(self, n, M, pitch, fh, fw, pool, steps, out_h, out_w, out_dil):
        self.n, self.M, self.pitch, self.fh, self.fw, self.pool = n, M, pitch, fh, fw, pool
        self.steps = steps
        self.elements = [pow(3, s, 2 * n) for s in steps]
        self.out_h, self.out_w, self.out_dil = out_h, out_w, out_dil
        self.valid = [out_dil * (y * pitch + x) for y in range(out_h) for x in range(out_w)]

    def fold(self, w, t):
        """[Cout][Cin][fh][fw] integers -> [Cout][Cin][T] in [0, t): w'[a][b] = Sum_{u, v < pool} w[a - u][b - v] mod t, the pool's window sum folded into the taps"""
        w = np.asarray(w)
        if w.ndim != 4 or w.shape[2:] != (self.fh, self.fw):
            raise ValueError("ConvSlotsPlan.fold: weights must be [Cout][Cin][fh][fw]")
        p, t = self.pool, int(t)
        out = np.zeros(w.shape[:2] + (self.fh + p - 1, self.fw + p - 1), dtype=object)
        wm = w.astype(object) % t
        for u in range(p):
            for v in range(p):
                out[:, :, u:u + self.fh, v:v + self.fw] += wm
        return (out % t).astype(np.int64).reshape(w.shape[0], w.shape[1], -1)


def conv_slots_plan(n, M, pitch, H, W, fh, fw, dil=1, pool=1):
    """A 'valid' convolution (stride 1 on the dilated grid, then a pool x pool sum pool of stride pool) of ONE image whose channel planes each fill a ciphertext:
    pixel (y, x) of an H x W plane at slot dil (y pitch + x), tiled with period M over both rows of n/2 slots (matvecSlots' input contract; M a power of two
    <= n/2 that the plane fits in).  Tap (a, b) is the row rotation by dil (a pitch + b), so output (y, x) lands where input (y, x) was -- with a pool, where input
    (pool y, pool x) was: dilation dil pool, the same pitch.  Slots outside `valid` hold junk that the next layer never reads: no masks, no zero padding.
    Raises ValueError for a plane that does not fit, a step >= n/2, M not a power of two, or a window larger than the plane"""
    n, M, pitch, H, W, fh, fw, dil, pool = (int(v) for v in (n, M, pitch, H, W, fh, fw, dil, pool))
    if n < 2 or n & (n - 1) or M < 1 or M & (M - 1) or M > n // 2:
        raise ValueError("conv_slots_plan: M must be a power of two <= n/2")
    if min(pitch, H, W, fh, fw, dil, pool) < 1 or W > pitch or fh > H or fw > W or dil * ((H - 1) * pitch + W - 1) >= M:
        raise ValueError("conv_slots_plan: the plane does not fit (W <= pitch, dil ((H - 1) pitch + W - 1) < M, window <= plane)")
    out_h, out_w = (H - fh + 1) // pool, (W - fw + 1) // pool
    if out_h < 1 or out_w < 1:
        raise ValueError("conv_slots_plan: the pool leaves no output")
    steps = [dil * (a * pitch + b) for a in range(fh + pool - 1) for b in range(fw + pool - 1)]
    if steps[-1] >= n // 2:
        raise ValueError("conv_slots_plan: a tap's step reaches n/2")
    return ConvSlotsPlan(n, M, pitch, fh, fw, pool, steps, out_h, out_w, dil * pool)


class ConvSlotsGeomPlan:
    """What conv_slots_plan_geom returns.  steps [T]: the row rotation of every tap of the (fh + stride (pool - 1)) x (fw + stride (pool - 1)) window, row-major,
    negative for a right rotation; elements [T]: crc_galois_elt_rows(step); out_h, out_w, out_dil: output (y, x) at slot origin + out_dil (y pitch + x) of every
    period M; valid: those slots of the first period, row-major; needs_clean_input: pad > 0 -- every slot of a period that holds no pixel must hold exactly 0.
    fold(w, t): the weights the taps take; mask_slots(): the 0/1 slot vector of the valid outputs"""
    def __init__(self, n, M, pitch, origin, fh, fw, pad, stride, pool, pool_stride, steps, out_h, out_w, out_dil):
        self.n, self.M, self.pitch, self.origin, self.fh, self.fw = n, M, pitch, origin, fh, fw
        self.pad, self.stride, self.pool, self.pool_stride = pad, stride, pool, pool_stride
        self.steps = steps
        self.elements = [pow(3, s if s >= 0 else n // 2 + s, 2 * n) for s in steps]
        self.out_h, self.out_w, self.out_dil = out_h, out_w, out_dil
        self.needs_clean_input = pad > 0
        self.valid = [origin + out_dil * (y * pitch + x) for y in range(out_h) for x in range(out_w)]

    def fold(self, w, t):
        """[Cout][Cin][fh][fw] integers -> [Cout][Cin][T] in [0, t): w'[a][b] = Sum_{u, v < pool} w[a - stride u][b - stride v] mod t"""
        w = np.asarray(w)
        if w.ndim != 4 or w.shape[2:] != (self.fh, self.fw):
            raise ValueError("ConvSlotsGeomPlan.fold: weights must be [Cout][Cin][fh][fw]")
        p, s, t = self.pool, self.stride, int(t)
        out = np.zeros(w.shape[:2] + (self.fh + s * (p - 1), self.fw + s * (p - 1)), dtype=object)
        wm = w.astype(object) % t
        for u in range(p):
            for v in range(p):
                out[:, :, s * u:s * u + self.fh, s * v:s * v + self.fw] += wm
        return (out % t).astype(np.int64).reshape(w.shape[0], w.shape[1], -1)

    def mask_slots(self, n=None):
        """int64 [n]: 1 exactly where (slot mod M) is in valid -- the plaintext slots of conv_slots_bias_mask's mask row"""
        n = self.n if n is None else int(n)
        if n % self.M:
            raise ValueError("ConvSlotsGeomPlan.mask_slots: n must be a multiple of M")
        row = np.zeros(self.M, dtype=np.int64)
        row[self.valid] = 1
        return np.tile(row, n // self.M)


def conv_slots_plan_geom(n, M, pitch, origin, H, W, fh, fw, dil=1, pad=0, stride=1, pool=1, pool_stride=0):
    """conv_slots_plan with an origin, `pad` zero pixels on every side, a conv stride and a pool x pool sum pool of stride pool_stride (0: pool) on the convolution's
    outputs: pixel (y, x) at slot origin + dil (y pitch + x) of every period M; tap (a, b) is the row rotation by dil ((a - pad) pitch + (b - pad)); output (y, x)
    lands at origin + dil stride pool_stride (y pitch + x).  pad = 0: non-pixel slots may hold anything.  pad > 0: they must hold exactly 0 (needs_clean_input).
    Raises ValueError for what conv_slots_plan refuses, for outputs that leave the period or share a slot, and -- by enumeration over every tap of every valid
    output -- for a tap beyond the plane's edge that lands on another pixel's slot modulo M (too little margin).  With pad = 0, stride = 1, pool_stride = pool and
    origin = 0 it is conv_slots_plan"""
    n, M, pitch, origin, H, W, fh, fw, dil, pad, stride, pool, ps = (int(v) for v in (n, M, pitch, origin, H, W, fh, fw, dil, pad, stride, pool, pool_stride))
    if n < 2 or n & (n - 1) or M < 1 or M & (M - 1) or M > n // 2:
        raise ValueError("conv_slots_plan_geom: M must be a power of two <= n/2")
    ps = ps or pool
    if min(pitch, H, W, fh, fw, dil, stride, pool, ps) < 1 or pad < 0 or origin < 0 or W > pitch or max(pitch, origin, H, W, fh, fw, dil, pad, stride, pool, ps) > M \
            or origin + dil * ((H - 1) * pitch + W - 1) >= M or fh > H + 2 * pad or fw > W + 2 * pad:
        raise ValueError("conv_slots_plan_geom: the plane does not fit (W <= pitch, origin + dil ((H - 1) pitch + W - 1) < M, window <= padded plane)")
    ch, cw = (H + 2 * pad - fh) // stride + 1, (W + 2 * pad - fw) // stride + 1
    if ch < pool or cw < pool:
        raise ValueError("conv_slots_plan_geom: the pool leaves no output")
    oh, ow = (ch - pool) // ps + 1, (cw - pool) // ps + 1
    eh, ew, od = fh + stride * (pool - 1), fw + stride * (pool - 1), dil * stride * ps
    if od > 0x7fffffff or origin + od * ((oh - 1) * pitch + ow - 1) >= M:
        raise ValueError("conv_slots_plan_geom: an output lands beyond the period")
    steps = [dil * ((a - pad) * pitch + (b - pad)) for a in range(eh) for b in range(ew)]
    if max(abs(s) for s in steps) >= n // 2:
        raise ValueError("conv_slots_plan_geom: a tap's step reaches n/2")
    plan = ConvSlotsGeomPlan(n, M, pitch, origin, fh, fw, pad, stride, pool, ps, steps, oh, ow, od)
    if len(set(plan.valid)) != len(plan.valid):
        raise ValueError("conv_slots_plan_geom: two outputs share a slot")
    pixel = {origin + dil * (y * pitch + x) for y in range(H) for x in range(W)}
    for y in range(oh if pad else 0):
        for x in range(ow):
            for a in range(eh):
                for b in range(ew):
                    iy, ix = stride * ps * y + a - pad, stride * ps * x + b - pad
                    if not (0 <= iy < H and 0 <= ix < W) and (plan.valid[y * ow + x] + steps[a * ew + b]) % M in pixel:
                        raise ValueError("conv_slots_plan_geom: too little margin -- a tap beyond the plane's edge lands on a pixel's slot")
    return plan


class DensePlanesPlan:
    """What dense_planes_plan returns.  steps [R]: the distinct values (in_slots[p] - out_slots[o]) mod M, ascending; elements [R]: 3^step mod 2n
    (crc_galois_elt_rows; step 0 is the element 1, which needs no key).  fold(W, t): the plaintext rows the steps take"""
    def __init__(self, n, M, in_slots, out_slots):
        self.n, self.M, self.in_slots, self.out_slots = n, M, list(in_slots), list(out_slots)
        self.steps = sorted({(p - o) % M for p in self.in_slots for o in self.out_slots})
        self.elements = [pow(3, s, 2 * n) for s in self.steps]

    def fold(self, W, t, j=None):
        """W [O][Cin][P] integers (any int64, taken mod t) -> slot rows [R][Cin][n] in [0, t) -- or [Cin][n] of the one step j, for a layer whose R Cin n integers
        should not exist at once: for i mod M = in_slots[p], rows[j][c][i] = W[o][c][p] where out_slots[o] = (in_slots[p] - steps[j]) mod M; 0 where no such o
        exists and at every other slot"""
        W = np.asarray(W)
        O, P = len(self.out_slots), len(self.in_slots)
        if W.ndim != 3 or W.shape[0] != O or W.shape[2] != P or W.shape[1] < 1 or int(t) < 2:
            raise ValueError("DensePlanesPlan.fold: weights must be [O][Cin][P] and t >= 2")
        Wm = (W.astype(object) % int(t)).astype(np.int64)
        at = {o: i for i, o in enumerate(self.out_slots)}

        def one(step):
            base = np.zeros((W.shape[1], self.M), dtype=np.int64)
            for p, sp in enumerate(self.in_slots):
                o = at.get((sp - step) % self.M)
                if o is not None:
                    base[:, sp] = Wm[o, :, p]
            return np.tile(base, (1, self.n // self.M))
        if j is not None:
            return one(self.steps[j])
        return np.stack([one(s) for s in self.steps])


def dense_planes_plan(n, M, in_slots, out_slots):
    """A dense layer behind packed channel planes, rotating its OUTPUTS: Cin ciphertexts x_c whose valid entries sit at the slots in_slots [P] of every period M
    (tiled over both rows of n/2 slots: matvecSlots' contract; every other slot may hold junk), O outputs that land at out_slots [O] (an int O means 0 .. O - 1):
        y = Sum_j rotate_rows( Sum_c rows[j][c] (.) x_c, steps[j] )   holds   Sum_c Sum_p W[o][c][p] x_c[in_slots[p]]   at out_slots[o]
    and exactly 0 at every other slot of the period (rotate_rows' convention: after a rotation by r, slot i holds old slot (i + r) mod n/2).  The choice of
    out_slots decides the number of steps.  Raises ValueError for M not a power of two <= n/2, an empty or duplicated slot list, a slot outside [0, M)"""
    n, M = int(n), int(M)
    if isinstance(out_slots, (int, np.integer)):
        out_slots = range(int(out_slots))
    in_slots, out_slots = [int(v) for v in in_slots], [int(v) for v in out_slots]
    if n < 2 or n & (n - 1) or M < 1 or M & (M - 1) or M > n // 2:
        raise ValueError("dense_planes_plan: M must be a power of two <= n/2")
    for name, sl in (("in_slots", in_slots), ("out_slots", out_slots)):
        if not sl or len(set(sl)) != len(sl) or min(sl) < 0 or max(sl) >= M:
            raise ValueError(f"dense_planes_plan: {name} must be a non-empty list of distinct slots of [0, M)")
    return DensePlanesPlan(n, M, in_slots, out_slots)


def h5_read(path, name):
    L = load()
    cnt = SZ(0)
    _chk(L.crc_h5_dataset_count(path.encode(), name.encode(), ctypes.byref(cnt)), f"crc_h5_dataset_count({name})")
    out = np.zeros(cnt.value, dtype=np.float32)
    _chk(L.crc_h5_read_f32(path.encode(), name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), cnt.value, None), "crc_h5_read_f32")
    return out


def h5_count(path, name):
    """number of elements of a dataset"""
    cnt = SZ(0)
    _chk(load().crc_h5_dataset_count(path.encode(), name.encode(), ctypes.byref(cnt)), f"crc_h5_dataset_count({name})")
    return int(cnt.value)


def h5_list(path):
    L = load()
    buf = ctypes.create_string_buffer(1 << 16)
    _chk(L.crc_h5_list(path.encode(), buf, len(buf)), "crc_h5_list")
    return [s for s in buf.value.decode().split("\n") if s]


class DBuf:
    """a device allocation owned through crc_malloc/crc_free"""

    def __init__(self, eng, nbytes):
        self.eng, self.nbytes = eng, int(nbytes)
        p = VP()
        _chk(eng.L.crc_malloc(eng.c, max(self.nbytes, 8), ctypes.byref(p)), "crc_malloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.eng.L.crc_free(self.eng.c, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """One context = one (n, q[], t) parameter set on one device (device=-1: host-only, for encode/client/tables)."""

    def __init__(self, n, q, t, device=0, _level_of=None):
        self.L = load()
        self.n, self.k, self.t, self.device = int(n), len(q), int(t), device
        self.q = np.array(q, dtype=np.uint64)
        c = VP()
        if _level_of is None:
            _chk(self.L.crc_ctx_create(self.n, _pu(self.q), self.k, self.t, device, ctypes.byref(c)), "crc_ctx_create")
        else:       # (derived_level: the first len(q) moduli of that engine, its key-switching gadget kept)
            _chk(self.L.crc_ctx_create_level(_level_of.c, self.k, device, ctypes.byref(c)), "crc_ctx_create_level")
        self.c = c
        self.kbsk = self.L.crc_ctx_kbsk(self.c)
        self.stream = None

    def close(self):
        if self.c:
            self.L.crc_ctx_destroy(self.c)
            self.c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory
    def mem_info(self):
        f, t = SZ(0), SZ(0)
        _chk(self.L.crc_mem_info(self.c, ctypes.byref(f), ctypes.byref(t)), "crc_mem_info")
        return f.value, t.value

    def alloc(self, nbytes):
        return DBuf(self, nbytes)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        b = DBuf(self, arr.nbytes)
        _chk(self.L.crc_memcpy_h2d(self.c, b.ptr, arr.ctypes.data, arr.nbytes, self.stream), "crc_memcpy_h2d")
        self.sync()
        return b

    def download(self, buf, shape, dtype=np.uint64):
        out = np.zeros(shape, dtype=dtype)
        self.sync()
        _chk(self.L.crc_memcpy_d2h(self.c, out.ctypes.data, buf.ptr if isinstance(buf, DBuf) else buf, out.nbytes, self.stream), "crc_memcpy_d2h")
        self.sync()
        return out

    def sync(self):
        _chk(self.L.crc_stream_sync(self.c, self.stream), "crc_stream_sync")

    def set_tuning(self, name, value):
        """tools / tests only: change one tuning switch of this (quiescent) context (the environment is read once, at creation)"""
        self.sync()
        _chk(self.L.crc_ctx_set_tuning(self.c, name.encode(), int(value)), f"crc_ctx_set_tuning({name})")

    def table(self, name, cap=1 << 16):
        out = np.zeros(cap, dtype=np.uint64)
        cnt = _chk(self.L.crc_ctx_table(self.c, name.encode(), _pu(out), cap), f"crc_ctx_table({name})")
        return out[:cnt].copy()

    # ---- modulus switching: continue over the first `kept` moduli (crc_mod_switch*)
    def level(self, kept):
        """a second Engine over the first `kept` moduli: same n, t and device.  Rows [0, kept) of this engine's NTT-form secret key, public key and plaintext rows
        are valid there; evaluation and Galois keys are generated afresh on it (gen_evk / gen_galois_keys with the prefix secret-key rows)"""
        kept = int(kept)
        if not 1 <= kept < self.k:
            raise ValueError(f"level({kept}): a level keeps 1 .. {self.k - 1} of the {self.k} moduli")
        return Engine(self.n, [int(v) for v in self.q[:kept]], self.t, device=self.device)

    # ---- a level WITHOUT the secret key: the gadget of the key switch stays this engine's, and this engine's keys, restricted, are the level's (crc_keys_restrict*)
    def derived_level(self, kept):
        """an Engine over the first `kept` moduli made by crc_ctx_create_level: as level(kept) for everything but key switching, which takes this engine's evaluation
        and Galois keys restricted to the level (keys_restrict[_dev], seeded_keys_expand_level[_dev]).  Key generation is refused on it"""
        kept = int(kept)
        if not 1 <= kept < self.k:
            raise ValueError(f"derived_level({kept}): a level keeps 1 .. {self.k - 1} of the {self.k} moduli")
        return Engine(self.n, [int(v) for v in self.q[:kept]], self.t, device=self.device, _level_of=self)

    @property
    def key_moduli(self):
        """modulus count of the key-switching gadget: k, or on a derived level the top ancestor's k"""
        return self.L.crc_ctx_key_moduli(self.c)

    def keys_restrict_supported(self, to):
        return bool(self.L.crc_keys_restrict_supported(self.c, to.c))

    def keys_restrict(self, to, keys, dbc=16):
        """host twin: blobs [n_keys][crc_evk_words] of this engine (evaluation, Galois or conjugated) -> [n_keys][crc_evk_words] of the derived level `to`"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.L.crc_evk_words(self.c, dbc))
        out = np.zeros((keys.shape[0], to.L.crc_evk_words(to.c, dbc)), dtype=np.uint64)
        _chk(self.L.crc_keys_restrict(self.c, to.c, _pu(keys), keys.shape[0], dbc, _pu(out)), "crc_keys_restrict")
        return out

    def keys_restrict_dev(self, to, d_keys, n_keys, d_out, dbc=16):
        _chk(self.L.crc_keys_restrict_dev(self.c, to.c, self.p(d_keys), n_keys, dbc, self.p(d_out), self.stream), "crc_keys_restrict_dev")

    def seeded_keys_expand_level(self, to, first, ids, public_seed, dbc=16, conjugate=False):
        """host twin: this engine's seeded rows -> the blobs of the derived level `to`, = keys_restrict(to, seeded_keys_expand(...))"""
        ids = self._elts(ids)
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(ids.size, self.seeded_key_words(dbc))
        out = np.zeros((ids.size, to.L.crc_evk_words(to.c, dbc)), dtype=np.uint64)
        _chk(self.L.crc_seeded_keys_expand_level(self.c, to.c, _pu(first), _pu(ids), ids.size, dbc, self._key(public_seed), 1 if conjugate else 0, _pu(out)),
             "crc_seeded_keys_expand_level")
        return out

    def seeded_keys_expand_level_dev(self, to, d_first, ids, public_seed, d_out, dbc=16, conjugate=False):
        ids = self._elts(ids)
        _chk(self.L.crc_seeded_keys_expand_level_dev(self.c, to.c, self.p(d_first), _pu(ids), ids.size, dbc, self._key(public_seed), 1 if conjugate else 0,
                                                     self.p(d_out), self.stream), "crc_seeded_keys_expand_level_dev")

    def mod_switch_supported(self, to):
        return bool(self.L.crc_mod_switch_supported(self.c, to.c))

    def mod_switch_work_bytes(self, to, count, size=2, in_form=COEFF, out_form=COEFF):
        return self.L.crc_mod_switch_work_bytes(self.c, to.c, count, size, in_form, out_form)

    def mod_switch_dev(self, to, d_in, count, d_out, d_work, size=2, in_form=COEFF, out_form=COEFF):
        """d_in [count][size][k][n] of this engine -> d_out [count][size][to.k][n] of `to`, on this engine's stream"""
        _chk(self.L.crc_mod_switch_forms(self.c, to.c, self.p(d_in), in_form, count, size, self.p(d_out), out_form, self.p(d_work), self.stream),
             "crc_mod_switch_forms")

    def mod_switch(self, to, cts, size=2, in_form=COEFF, out_form=COEFF):
        """host twin: ciphertexts [count][size][k][n] -> [count][size][to.k][n]"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, size, self.k, self.n)
        out = np.zeros((cts.shape[0], size, to.k, self.n), dtype=np.uint64)
        _chk(self.L.crc_mod_switch(self.c, to.c, _pu(cts), in_form, cts.shape[0], size, _pu(out), out_form), "crc_mod_switch")
        return out

    # ---- noise flooding: sanitise a response before it leaves (crc_flood*)
    def flood_supported(self, flood_bits):
        return bool(self.L.crc_flood_supported(self.c, flood_bits))

    def flood_bits(self, budget_bits_in, lambda_bits=40):
        """the smallest admitted B that covers, by lambda_bits, the noise of a ciphertext with budget_bits_in bits of budget -- the A-PRIORI budget of the
        network, never a measured one"""
        return _chk(self.L.crc_flood_bits(self.c, budget_bits_in, lambda_bits), "crc_flood_bits")

    def flood_budget_bound(self, budget_bits_in, flood_bits):
        return _chk(self.L.crc_flood_budget_bound(self.c, budget_bits_in, flood_bits), "crc_flood_budget_bound")

    def flood_dev_work_bytes(self, count, form=COEFF):
        return self.L.crc_flood_dev_work_bytes(self.c, count, form)

    def flood_dev(self, d_pk, d_ct, count, flood_bits, d_work, form=COEFF, seed=None, key=None, stream_base=0):
        """d_ct [count][2][k][n] in `form`, flooded in place on this engine's stream.  `key` (32 bytes) with `stream_base`, or a public `seed` (tests)"""
        self._seeded_or_keyed("flood_dev", (self.c, self.p(d_pk), self.p(d_ct), count, form, flood_bits), seed, key, stream_base, (self.p(d_work), self.stream))

    def flood(self, pk, cts, flood_bits, form=COEFF, seed=None, key=None, stream_base=0):
        """host twin: a flooded copy of ciphertexts [count][2][k][n]"""
        out = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2, self.k, self.n).copy()
        pk = np.ascontiguousarray(pk, dtype=np.uint64)
        self._seeded_or_keyed("flood", (self.c, _pu(pk), _pu(out), out.shape[0], form, flood_bits), seed, key, stream_base, ())
        return out

    # ---- host side: encode / client
    def encode(self, values, dtype=np.float32):
        values = np.ascontiguousarray(np.asarray(values, dtype=dtype).reshape(-1))
        out = np.zeros((values.size, self.n), dtype=np.uint64)
        cc = np.zeros(values.size, dtype=np.int32)
        if dtype == np.float32:
            _chk(self.L.crc_encode_f32(self.c, values.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), values.size, _pu(out), cc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "crc_encode_f32")
        else:
            _chk(self.L.crc_encode_f64(self.c, values.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), values.size, _pu(out), cc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "crc_encode_f64")
        return out, cc

    COMPACT_WORDS = 96        # CRC_PLAIN_COMPACT_WORDS

    def encode_to_device(self, values, d_plain, d_compact):
        """float32 weights -> dense coefficient-form plaintexts [count][n] at d_plain: encoded in compact form on the host threads (96 words per weight, the only
        coefficients the encoder sets), copied down as they are and zero-extended on the device.  d_compact: count * 96 * 8 bytes of device staging"""
        values = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
        cp = np.empty((values.size, self.COMPACT_WORDS), dtype=np.uint64)
        _chk(self.L.crc_encode_f32_compact(self.c, values.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), values.size, _pu(cp), None), "crc_encode_f32_compact")
        _chk(self.L.crc_memcpy_h2d(self.c, self.p(d_compact), cp.ctypes.data, cp.nbytes, self.stream), "crc_memcpy_h2d")
        _chk(self.L.crc_plain_expand(self.c, self.p(d_compact), values.size, self.p(d_plain), self.stream), "crc_plain_expand")
        self.sync()             # cp is the source of an asynchronous copy until here
        return values.size

    def decode(self, plain):
        return self.L.crc_decode(self.c, _pu(np.ascontiguousarray(plain)))

    # ---- slot batching: n numbers of Z_t per plaintext (prime t = 1 mod 2n); (item c, slot i) at values[c * item_stride + i * slot_stride]
    @property
    def slots_supported(self):
        return bool(self.L.crc_slots_supported(self.c))

    @staticmethod
    def slots_prime(n, bits):
        """the largest prime below 2**bits that is 1 mod 2n"""
        t = u64(0)
        _chk(load().crc_slots_prime(int(n), int(bits), ctypes.byref(t)), "crc_slots_prime")
        return int(t.value)

    def slots_compose(self, values, count, slots, item_stride, slot_stride):
        """host twin: int64 values (flat, strided) -> plaintexts [count][n]"""
        values = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
        assert values.size > (count - 1) * item_stride + (slots - 1) * slot_stride
        out = np.zeros((count, self.n), dtype=np.uint64)
        _chk(self.L.crc_slots_compose(self.c, values.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), count, slots, item_stride, slot_stride, _pu(out)),
             "crc_slots_compose")
        return out

    def slots_decompose(self, plains, slots, item_stride, slot_stride, size=None):
        """host twin: plaintexts [count][n] -> flat int64 array of `size` words (default: just what the strides reach), untouched words 0"""
        plains = np.ascontiguousarray(plains, dtype=np.uint64).reshape(-1, self.n); count = plains.shape[0]
        need = (count - 1) * item_stride + (slots - 1) * slot_stride + 1
        out = np.zeros(need if size is None else size, dtype=np.int64)
        assert out.size >= need
        _chk(self.L.crc_slots_decompose(self.c, _pu(plains), count, slots, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), item_stride, slot_stride),
             "crc_slots_decompose")
        return out

    def slots_compose_dev(self, d_values, count, slots, item_stride, slot_stride, d_plain):
        _chk(self.L.crc_slots_compose_dev(self.c, self.p(d_values), count, slots, item_stride, slot_stride, self.p(d_plain), self.stream), "crc_slots_compose_dev")

    def slots_decompose_dev(self, d_plain, count, slots, d_values, item_stride, slot_stride):
        _chk(self.L.crc_slots_decompose_dev(self.c, self.p(d_plain), count, slots, self.p(d_values), item_stride, slot_stride, self.stream),
             "crc_slots_decompose_dev")

    def slots_rescale(self, plains, divisor):
        """host twin: every slot of plaintexts [count][n] -> floor(slot / divisor + 1/2), recomposed"""
        plains = np.ascontiguousarray(plains, dtype=np.uint64).reshape(-1, self.n)
        out = np.zeros_like(plains)
        _chk(self.L.crc_slots_rescale(self.c, _pu(plains), plains.shape[0], int(divisor), _pu(out)), "crc_slots_rescale")
        return out

    def slots_rescale_dev(self, d_plain_in, count, divisor, d_plain_out):
        _chk(self.L.crc_slots_rescale_dev(self.c, self.p(d_plain_in), count, int(divisor), self.p(d_plain_out), self.stream), "crc_slots_rescale_dev")

    def slots_refresh_dev_work_bytes(self, count, in_form=COEFF):
        return self.L.crc_slots_refresh_dev_work_bytes(self.c, count, in_form)

    def slots_refresh_dev(self, d_sk, d_pk, d_ct_in, count, divisor, seed, d_ct_out, d_work, in_form=COEFF, out_form=COEFF, key=None, stream_base=0):
        """decrypt -> rescale every slot by `divisor` -> encrypt under the public key: crc_decrypt_dev, crc_slots_rescale_dev, crc_encrypt_dev[_key]_forms as one call"""
        self._seeded_or_keyed("slots_refresh_dev", (self.c, self.p(d_sk), self.p(d_pk), self.p(d_ct_in), count, in_form, int(divisor)), seed, key, stream_base,
                              (out_form, self.p(d_ct_out), self.p(d_work), self.stream))

    def slots_refresh_sym_dev_work_bytes(self, count, in_form=COEFF):
        return self.L.crc_slots_refresh_sym_dev_work_bytes(self.c, count, in_form)

    def slots_refresh_sym_dev(self, d_sk, d_ct_in, count, divisor, seed, d_ct_out, d_work, in_form=COEFF, out_form=COEFF, key=None, stream_base=0):
        """the same under the secret key (crc_encrypt_sym_dev[_key]_forms)"""
        self._seeded_or_keyed("slots_refresh_sym_dev", (self.c, self.p(d_sk), self.p(d_ct_in), count, in_form, int(divisor)), seed, key, stream_base,
                              (out_form, self.p(d_ct_out), self.p(d_work), self.stream))

    # client-side activation: window = (xd, yd, xs, ys, xf, yf); outputs ((xd - xf) // xs + 1) x ((yd - yf) // ys + 1) rows per plane
    def slots_act(self, plains, planes, window, divisor, relu=0, cap=0):
        """host twin: plaintexts [planes][xd][yd][n] -> [planes][xo][yo][n]; per slot the window's maximum, floor(m / divisor + 1/2), ReLU, cap, recomposed"""
        xd, yd, xs, ys, xf, yf = window
        plains = np.ascontiguousarray(plains, dtype=np.uint64).reshape(planes * xd * yd, self.n)
        xo, yo = ((xd - xf) // xs + 1, (yd - yf) // ys + 1) if xs > 0 and ys > 0 else (0, 0)
        out = np.zeros((max(planes * xo * yo, 0), self.n), dtype=np.uint64)
        _chk(self.L.crc_slots_act(self.c, _pu(plains), planes, xd, yd, xs, ys, xf, yf, int(divisor), int(relu), int(cap), _pu(out)), "crc_slots_act")
        return out

    def slots_act_dev(self, d_plain_in, planes, window, divisor, relu, cap, d_plain_out):
        _chk(self.L.crc_slots_act_dev(self.c, self.p(d_plain_in), planes, *window, int(divisor), int(relu), int(cap), self.p(d_plain_out), self.stream),
             "crc_slots_act_dev")

    def slots_refresh_act_dev_work_bytes(self, planes, window, in_form=COEFF):
        return self.L.crc_slots_refresh_act_dev_work_bytes(self.c, planes, *window, in_form)

    def slots_refresh_act_dev(self, d_sk, d_pk, d_ct_in, planes, window, divisor, relu, cap, seed, d_ct_out, d_work, in_form=COEFF, out_form=COEFF, key=None,
                              stream_base=0):
        """decrypt planes * xd * yd ciphertexts -> slots_act_dev -> encrypt the planes * xo * yo outputs under the public key, as one call"""
        self._seeded_or_keyed("slots_refresh_act_dev", (self.c, self.p(d_sk), self.p(d_pk), self.p(d_ct_in), planes, *window, in_form, int(divisor), int(relu), int(cap)),
                              seed, key, stream_base, (out_form, self.p(d_ct_out), self.p(d_work), self.stream))

    def slots_refresh_act_sym_dev_work_bytes(self, planes, window, in_form=COEFF):
        return self.L.crc_slots_refresh_act_sym_dev_work_bytes(self.c, planes, *window, in_form)

    def slots_refresh_act_sym_dev(self, d_sk, d_ct_in, planes, window, divisor, relu, cap, seed, d_ct_out, d_work, in_form=COEFF, out_form=COEFF, key=None,
                                  stream_base=0):
        """the same under the secret key"""
        self._seeded_or_keyed("slots_refresh_act_sym_dev", (self.c, self.p(d_sk), self.p(d_ct_in), planes, *window, in_form, int(divisor), int(relu), int(cap)),
                              seed, key, stream_base, (out_form, self.p(d_ct_out), self.p(d_work), self.stream))

    def keygen(self, seed):
        sk = np.zeros((self.k, self.n), dtype=np.uint64); pk = np.zeros((2, self.k, self.n), dtype=np.uint64)
        _chk(self.L.crc_keygen(self.c, seed, _pu(sk), _pu(pk)), "crc_keygen"); return sk, pk

    def gen_evk(self, seed, sk, dbc=16):
        evk = np.zeros(self.L.crc_evk_words(self.c, dbc), dtype=np.uint64)
        _chk(self.L.crc_gen_evk(self.c, seed, _pu(sk), dbc, _pu(evk)), "crc_gen_evk"); return evk

    def encrypt(self, pk, plains, seed):
        plains = np.ascontiguousarray(plains); lead = plains.shape[:-1]
        cnt = int(np.prod(lead)) if lead else 1
        ct = np.zeros((cnt, 2, self.k, self.n), dtype=np.uint64)
        _chk(self.L.crc_encrypt(self.c, _pu(pk), _pu(plains.reshape(cnt, self.n)), cnt, seed, _pu(ct)), "crc_encrypt")
        return ct.reshape(lead + (2, self.k, self.n))

    # key-based client side (ChaCha20 under a 256-bit key; `key` = 32 bytes, random_key() draws it from the OS)
    @staticmethod
    def _key(key):
        key = bytes(key)
        assert len(key) == 32
        return (ctypes.c_uint8 * 32).from_buffer_copy(key)

    def _seeded_or_keyed(self, name, head, seed, key, stream_base, tail):
        """crc_<name>(*head, seed, *tail), or with `key` crc_<name>_key(*head, key, stream_base, *tail): the two randomness forms of one entry point"""
        if key is None:
            return _chk(getattr(self.L, "crc_" + name)(*head, seed, *tail), "crc_" + name)
        return _chk(getattr(self.L, "crc_" + name + "_key")(*head, self._key(key), stream_base, *tail), "crc_" + name + "_key")

    def random_key(self):
        buf = (ctypes.c_uint8 * 32)()
        _chk(self.L.crc_random_key(buf), "crc_random_key"); return bytes(buf)

    def keygen_key(self, key):
        sk = np.zeros((self.k, self.n), dtype=np.uint64); pk = np.zeros((2, self.k, self.n), dtype=np.uint64)
        _chk(self.L.crc_keygen_key(self.c, self._key(key), _pu(sk), _pu(pk)), "crc_keygen_key"); return sk, pk

    def gen_evk_key(self, key, sk, dbc=16):
        evk = np.zeros(self.L.crc_evk_words(self.c, dbc), dtype=np.uint64)
        _chk(self.L.crc_gen_evk_key(self.c, self._key(key), _pu(sk), dbc, _pu(evk)), "crc_gen_evk_key"); return evk

    def encrypt_key(self, pk, plains, key, stream_base=0):
        plains = np.ascontiguousarray(plains); lead = plains.shape[:-1]
        cnt = int(np.prod(lead)) if lead else 1
        ct = np.zeros((cnt, 2, self.k, self.n), dtype=np.uint64)
        _chk(self.L.crc_encrypt_key(self.c, _pu(pk), _pu(plains.reshape(cnt, self.n)), cnt, self._key(key), stream_base, _pu(ct)), "crc_encrypt_key")
        return ct.reshape(lead + (2, self.k, self.n))

    def encrypt_sym(self, sk, plains, seed, out_form=COEFF, key=None, stream_base=0):
        """encryption under the secret key on the host (crc_encrypt_sym; with `key`: crc_encrypt_sym_key) -- the bits the device entry points give"""
        plains = np.ascontiguousarray(plains); lead = plains.shape[:-1]
        cnt = int(np.prod(lead)) if lead else 1
        ct = np.zeros((cnt, 2, self.k, self.n), dtype=np.uint64)
        self._seeded_or_keyed("encrypt_sym", (self.c, _pu(sk), _pu(plains.reshape(cnt, self.n)), cnt), seed, key, stream_base, (out_form, _pu(ct)))
        return ct.reshape(lead + (2, self.k, self.n))

    # seeded secret-key ciphertexts: the c0 rows [count][k][n] (NTT form) and a PUBLIC 32-byte seed; c1 is regenerated from the seed
    def seeded_public_seed(self, seed):
        """the public seed the uint64 seed variant of encrypt_sym_seeded uses (crc_seeded_public_seed)"""
        buf = (ctypes.c_uint8 * 32)()
        _chk(self.L.crc_seeded_public_seed(seed, buf), "crc_seeded_public_seed"); return bytes(buf)

    def encrypt_sym_seeded(self, sk, plains, seed, key=None, public_seed=None, stream_base=0):
        """-> (c0 rows [..][k][n], public seed, stream_base).  With `key` (PRIVATE) and `public_seed`: crc_encrypt_sym_seeded_key; else the deterministic
        uint64 `seed` variant (tests, bench: NOT secure)"""
        plains = np.ascontiguousarray(plains); lead = plains.shape[:-1]
        cnt = int(np.prod(lead)) if lead else 1
        c0 = np.zeros((cnt, self.k, self.n), dtype=np.uint64)
        if key is None:
            _chk(self.L.crc_encrypt_sym_seeded(self.c, _pu(sk), _pu(plains.reshape(cnt, self.n)), cnt, seed, _pu(c0)), "crc_encrypt_sym_seeded")
            public_seed, stream_base = self.seeded_public_seed(seed), 0
        else:
            _chk(self.L.crc_encrypt_sym_seeded_key(self.c, _pu(sk), _pu(plains.reshape(cnt, self.n)), cnt, self._key(key), self._key(public_seed), stream_base,
                                                   _pu(c0)), "crc_encrypt_sym_seeded_key")
        return c0.reshape(lead + (self.k, self.n)), bytes(public_seed), stream_base

    def seeded_expand(self, c0, public_seed, stream_base=0, out_form=NTT):
        """the host twin of seeded_expand_dev: c0 [..][k][n] -> ciphertexts [..][2][k][n]"""
        c0 = np.ascontiguousarray(c0); lead = c0.shape[:-2]
        cnt = int(np.prod(lead)) if lead else 1
        ct = np.zeros((cnt, 2, self.k, self.n), dtype=np.uint64)
        _chk(self.L.crc_seeded_expand(self.c, _pu(c0), cnt, self._key(public_seed), stream_base, out_form, _pu(ct)), "crc_seeded_expand")
        return ct.reshape(lead + (2, self.k, self.n))

    def seeded_bytes(self, count):
        return self.L.crc_seeded_ct_bytes(self.c, count)

    def seeded_save(self, c0, public_seed, stream_base=0):
        c0 = np.ascontiguousarray(c0); cnt = c0.size // (self.k * self.n)
        buf = np.zeros(self.seeded_bytes(cnt), dtype=np.uint8); w = SZ(0)
        _chk(self.L.crc_seeded_ct_save(self.c, _pu(c0), cnt, self._key(public_seed), stream_base, buf.ctypes.data, buf.nbytes, ctypes.byref(w)), "crc_seeded_ct_save")
        return buf[:w.value].tobytes()

    def seeded_load(self, blob):
        """-> (c0 [count][k][n], public seed, stream_base); CrcError for a wrong hash, a short buffer or a count that does not match the length"""
        raw = np.frombuffer(bytes(blob), dtype=np.uint8).copy(); cnt = SZ(0)
        _chk(self.L.crc_seeded_ct_load(self.c, raw.ctypes.data, raw.nbytes, None, 0, ctypes.byref(cnt), None, None), "crc_seeded_ct_load")
        c0 = np.zeros((cnt.value, self.k, self.n), dtype=np.uint64); sd = (ctypes.c_uint8 * 32)(); base = u64(0)
        _chk(self.L.crc_seeded_ct_load(self.c, raw.ctypes.data, raw.nbytes, _pu(c0), cnt.value, ctypes.byref(cnt), sd, ctypes.byref(base)), "crc_seeded_ct_load")
        return c0, bytes(sd), base.value

    def decrypt(self, sk, cts, size=2):
        cts = np.ascontiguousarray(cts); lead = cts.shape[:-3]
        cnt = int(np.prod(lead)) if lead else 1
        out = np.zeros((cnt, self.n), dtype=np.uint64)
        _chk(self.L.crc_decrypt(self.c, _pu(sk), _pu(cts), cnt, size, _pu(out)), "crc_decrypt")
        return out.reshape(lead + (self.n,))

    def noise_budget(self, sk, ct):
        ct = np.ascontiguousarray(ct)
        return _chk(self.L.crc_noise_budget(self.c, _pu(sk), _pu(ct), ct.shape[-3]), "crc_noise_budget")

    # ---- device ops on DBuf / raw pointers (p(x) accepts DBuf, int, or torch tensor with data_ptr)
    @staticmethod
    def p(x):
        if x is None:
            return None
        if isinstance(x, DBuf):
            return x.ptr
        if hasattr(x, "data_ptr"):
            return x.data_ptr()
        return int(x)

    def plain_to_ntt(self, d_plain, count, d_out):
        _chk(self.L.crc_plain_to_ntt(self.c, self.p(d_plain), count, self.p(d_out), self.stream), "crc_plain_to_ntt")

    def plain_to_delta(self, d_plain, count, form, d_out):
        _chk(self.L.crc_plain_to_delta(self.c, self.p(d_plain), count, form, self.p(d_out), self.stream), "crc_plain_to_delta")

    def ntt_fwd(self, d_ct, count, size=2):
        _chk(self.L.crc_ntt_fwd(self.c, self.p(d_ct), count, size, self.stream), "crc_ntt_fwd")

    def ntt_fwd_box(self, d_src, d_dst, B, xd, yd, bxf, byf, xs, ys):
        """crc_ntt_fwd_box: [B][xd][yd] coefficient-form ciphertexts in, the NTT of their bxf x byf window sums at dilation (xs, ys) out ([B][xdo][ydo])"""
        _chk(self.L.crc_ntt_fwd_box(self.c, self.p(d_src), self.p(d_dst), B, xd, yd, bxf, byf, xs, ys, self.stream), "crc_ntt_fwd_box")

    def ntt_inv(self, d_ct, count, size=2):
        _chk(self.L.crc_ntt_inv(self.c, self.p(d_ct), count, size, self.stream), "crc_ntt_inv")

    def add(self, d_acc, d_b, count, size=2):
        _chk(self.L.crc_add(self.c, self.p(d_acc), self.p(d_b), count, size, self.stream), "crc_add")

    def add_plain(self, d_ct, d_delta, count, group, sign=1):
        _chk(self.L.crc_add_plain(self.c, self.p(d_ct), self.p(d_delta), count, group, sign, self.stream), "crc_add_plain")

    def multiply_plain_ntt(self, d_ct, d_w, count, group, size=2):
        _chk(self.L.crc_multiply_plain_ntt(self.c, self.p(d_ct), self.p(d_w), count, group, size, self.stream), "crc_multiply_plain_ntt")

    def multiply_plain(self, d_ct, d_w, count, group):
        _chk(self.L.crc_multiply_plain(self.c, self.p(d_ct), self.p(d_w), count, group, self.stream), "crc_multiply_plain")

    def conv2d_work_bytes(self, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form):
        return self.L.crc_conv2d_work_bytes(self.c, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form)

    def conv2d(self, d_x, d_w, d_bias, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, out_form, d_y, d_work, w_form=NTT):
        if w_form == NTT and in_form != NTTP and out_form != NTTP:
            _chk(self.L.crc_conv2d(self.c, self.p(d_x), self.p(d_w), self.p(d_bias), B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, out_form,
                                   self.p(d_y), self.p(d_work), self.stream), "crc_conv2d")
        else:
            _chk(self.L.crc_conv2d_forms(self.c, self.p(d_x), self.p(d_w), w_form, self.p(d_bias), B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, out_form,
                                         self.p(d_y), self.p(d_work), self.stream), "crc_conv2d_forms")

    # ---- limb form (CRC_NTTL): conv / dense on the matrix cores
    def limb_supported(self, zd, xf=1, yf=1):
        return bool(self.L.crc_limb_supported(self.c, zd, xf, yf))

    def limb_tensor_bytes(self, B, zd, xd=1, yd=1):
        return self.L.crc_limb_tensor_bytes(self.c, B, zd, xd, yd)

    def limb_weights_bytes(self, nf, zd, xf=1, yf=1):
        return self.L.crc_limb_weights_bytes(self.c, nf, zd, xf, yf)

    def limb_pack_weights(self, d_w_ntt, nf, zd, xf, yf, d_wl):
        _chk(self.L.crc_limb_pack_weights(self.c, self.p(d_w_ntt), nf, zd, xf, yf, self.p(d_wl), self.stream), "crc_limb_pack_weights")

    def plan_mac(self, zd, xd, yd, xs, ys, xf, yf, nf, B, matrix_cores=True):
        """the weight form (= kernel) of a conv / dense layer launched on B images (B = 0: shape only): crc_plan_mac, the policy shared with the C++ host classes"""
        wf = CI(0)
        _chk(self.L.crc_plan_mac(self.c, zd, xd, yd, xs, ys, xf, yf, nf, int(B or 0), 1 if matrix_cores else 0, ctypes.byref(wf)), "crc_plan_mac")
        return wf.value

    def plan_fold_pool(self, zd, xd, yd, xs, ys, xf, yf, nf, pxs, pys, pxf, pyf):
        f = CI(0)
        _chk(self.L.crc_plan_fold_pool(self.c, zd, xd, yd, xs, ys, xf, yf, nf, pxs, pys, pxf, pyf, ctypes.byref(f)), "crc_plan_fold_pool")
        return bool(f.value)

    def plan_hoist_pool(self, up, conv, pool, B, matrix_cores=True):
        """crc_plan_hoist_pool: is the pool behind a stride-1 convolution hoisted in front of it?  up: (zd, xd, yd, xs, ys, xf, yf, nf) of the layer in front as it
        runs (already folded), or None where no resident convolution feeds this one; conv: the same eight; pool: (xs, ys, xf, yf)"""
        h = CI(0)
        _chk(self.L.crc_plan_hoist_pool(self.c, *(tuple(up) if up else (0,) * 8), *conv, *pool, int(B or 0), 1 if matrix_cores else 0, ctypes.byref(h)),
             "crc_plan_hoist_pool")
        return bool(h.value)

    # ---- the box of a one-channel convolution: the layer reads the bxf x byf window sums of its input (crc_conv2d_box_forms); (xf, yf) is the BASE window
    def limb_conv1_box_supported(self, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf):
        return bool(self.L.crc_limb_conv1_box_supported(self.c, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf))

    def conv2d_box_forms_work_bytes(self, B, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf, in_form, w_form, out_form):
        return self.L.crc_conv2d_box_forms_work_bytes(self.c, B, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf, in_form, w_form, out_form)

    def conv2d_box(self, d_x, d_w, d_bias, B, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf, in_form, out_form, d_y, d_work, w_form=NTTL1):
        _chk(self.L.crc_conv2d_box_forms(self.c, self.p(d_x), self.p(d_w), w_form, self.p(d_bias), B, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf, in_form, out_form,
                                         self.p(d_y), self.p(d_work), self.stream), "crc_conv2d_box_forms")

    def plan_conv1_box(self, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf, B=0, matrix_cores=True):
        """crc_plan_conv1_box: does a one-channel layer with base window (xf, yf) sum its input (the box) instead of running the enlarged window?"""
        b = CI(0)
        _chk(self.L.crc_plan_conv1_box(self.c, zd, xd, yd, xs, ys, xf, yf, nf, bxf, byf, int(B or 0), 1 if matrix_cores else 0, ctypes.byref(b)),
             "crc_plan_conv1_box")
        return bool(b.value)

    # ---- scalar form (CRC_NTTLS): the layers of a slot-batched network, whose weights are constant polynomials
    def scalar_weights_bytes(self, nf, zd, xf=1, yf=1):
        return self.L.crc_scalar_weights_bytes(self.c, nf, zd, xf, yf)

    def scalar_supported(self, B, zd, xd, yd, xs, ys, xf, yf, nf):
        return bool(self.L.crc_scalar_supported(self.c, B, zd, xd, yd, xs, ys, xf, yf, nf))

    def scalar_pack_weights(self, d_w, w_stride, nf, zd, xf, yf, d_ws):
        """d_w: NTT-form weight rows (w_stride = n) or one residue per modulus [nf][zd][xf][yf][k] (w_stride = 1).  Returns False, with d_ws untouched, where a
        row is not a constant polynomial (crc_scalar_pack_weights' *constant = 0); any other failure raises"""
        const = CI(1)
        rc = self.L.crc_scalar_pack_weights(self.c, self.p(d_w), w_stride, nf, zd, xf, yf, self.p(d_ws), ctypes.byref(const), self.stream)
        if rc == -1 and const.value == 0:
            return False
        _chk(rc, "crc_scalar_pack_weights")
        return True

    def plan_mac_scalar(self, zd, xd, yd, xs, ys, xf, yf, nf, B):
        """crc_plan_mac for a layer of a slot-batched network: NTTLS where the scalar form runs (tuning key scalar_mac), else what plan_mac says"""
        wf = CI(0)
        _chk(self.L.crc_plan_mac_scalar(self.c, zd, xd, yd, xs, ys, xf, yf, nf, int(B or 0), ctypes.byref(wf)), "crc_plan_mac_scalar")
        return wf.value

    def limb_pack_weights_tile(self, d_w_tile, nf, f0, ft, zd, xf, yf, d_wl):
        _chk(self.L.crc_limb_pack_weights_tile(self.c, self.p(d_w_tile), nf, f0, ft, zd, xf, yf, self.p(d_wl), self.stream), "crc_limb_pack_weights_tile")

    def limb_pack_tensor(self, d_x, in_form, B, zd, xd, yd, d_xl):
        _chk(self.L.crc_limb_pack_tensor(self.c, self.p(d_x), in_form, B, zd, xd, yd, self.p(d_xl), self.stream), "crc_limb_pack_tensor")

    def limb_pack_tensor_at(self, d_x, in_form, B, zd, xd, yd, d_xl, Btot, b0):
        _chk(self.L.crc_limb_pack_tensor_at(self.c, self.p(d_x), in_form, B, zd, xd, yd, self.p(d_xl), Btot, b0, self.stream), "crc_limb_pack_tensor_at")

    # ---- one-channel convolutions on the matrix cores (weight form CRC_NTTL1)
    def limb_conv1_supported(self, zd, xd, yd, xs, ys, xf, yf, nf):
        return bool(self.L.crc_limb_conv1_supported(self.c, zd, xd, yd, xs, ys, xf, yf, nf))

    def limb_conv1_weights_bytes(self):
        return self.L.crc_limb_conv1_weights_bytes(self.c)

    def limb_conv1_weights_bytes_for(self, nf, xf, yf):
        return self.L.crc_limb_conv1_weights_bytes_for(self.c, nf, xf, yf)

    def limb_conv1_form(self, zd, xd, yd, xs, ys, xf, yf, nf):
        """0: not a one-channel matrix-core shape, 1: plane-major image, 2: pixel-major image (tuning key conv1_form)"""
        return self.L.crc_limb_conv1_form(self.c, zd, xd, yd, xs, ys, xf, yf, nf)

    def limb_conv1_pack_weights(self, d_w_ntt, nf, xf, yf, d_wl):
        _chk(self.L.crc_limb_conv1_pack_weights(self.c, self.p(d_w_ntt), nf, xf, yf, self.p(d_wl), self.stream), "crc_limb_conv1_pack_weights")

    def conv2d_forms_work_bytes(self, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, w_form, out_form):
        return self.L.crc_conv2d_forms_work_bytes(self.c, B, zd, xd, yd, xs, ys, xf, yf, nf, in_form, w_form, out_form)

    def pack28(self, d_rows, rows, unpack=False):
        _chk(self.L.crc_pack28(self.c, self.p(d_rows), rows, 1 if unpack else 0, self.stream), "crc_pack28")

    def conv2d_fold_pool(self, d_w, d_bias_ntt, d_div_ntt, nf, zd, xf, yf, cxs, cys, pxf, pyf, d_w_out, d_bias_out):
        _chk(self.L.crc_conv2d_fold_pool(self.c, self.p(d_w), self.p(d_bias_ntt), self.p(d_div_ntt), nf, zd, xf, yf, cxs, cys, pxf, pyf,
                                         self.p(d_w_out), self.p(d_bias_out), self.stream), "crc_conv2d_fold_pool")

    def conv2d_hoist_pool(self, d_w, d_bias_ntt, d_div_ntt, nf, zd, xf, yf, pxf, pyf, d_w_out, d_bias_out):
        _chk(self.L.crc_conv2d_hoist_pool(self.c, self.p(d_w), self.p(d_bias_ntt), self.p(d_div_ntt), nf, zd, xf, yf, pxf, pyf,
                                          self.p(d_w_out), self.p(d_bias_out), self.stream), "crc_conv2d_hoist_pool")

    def dense_work_bytes(self, B, in_dim, out_dim, in_form):
        return self.L.crc_dense_work_bytes(self.c, B, in_dim, out_dim, in_form)

    def dense(self, d_x, d_w, d_bias, B, in_dim, out_dim, in_form, out_form, d_y, d_work, w_form=NTT):
        if w_form == NTT and in_form != NTTP and out_form != NTTP:
            _chk(self.L.crc_dense(self.c, self.p(d_x), self.p(d_w), self.p(d_bias), B, in_dim, out_dim, in_form, out_form, self.p(d_y), self.p(d_work),
                                  self.stream), "crc_dense")
        else:
            _chk(self.L.crc_dense_forms(self.c, self.p(d_x), self.p(d_w), w_form, self.p(d_bias), B, in_dim, out_dim, in_form, out_form, self.p(d_y),
                                        self.p(d_work), self.stream), "crc_dense_forms")

    def pool(self, d_x, B, zd, xd, yd, xs, ys, xf, yf, d_div, form, d_y):
        _chk(self.L.crc_pool(self.c, self.p(d_x), B, zd, xd, yd, xs, ys, xf, yf, self.p(d_div), form, self.p(d_y), self.stream), "crc_pool")

    def pad(self, d_x, B, zd, xd, yd, px0, px1, py0, py1, form, d_y):
        """zero padding of the two spatial dimensions (crc_pad): [B][zd][xd][yd] -> [B][zd][px0 + xd + px1][py0 + yd + py1], the form (COEFF / NTT) kept"""
        _chk(self.L.crc_pad(self.c, self.p(d_x), B, zd, xd, yd, px0, px1, py0, py1, form, self.p(d_y), self.stream), "crc_pad")

    def batchnorm(self, d_x, B, zd, xd, yd, d_mean, d_invstd, form):
        _chk(self.L.crc_batchnorm(self.c, self.p(d_x), B, zd, xd, yd, self.p(d_mean), self.p(d_invstd), form, self.stream), "crc_batchnorm")

    def square_relin_work_bytes(self, count, dbc=16):
        return self.L.crc_square_relin_work_bytes(self.c, count, dbc)

    def square_relin(self, d_x, count, d_evk, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        _chk(self.L.crc_square_relin_forms(self.c, self.p(d_x), in_form, count, self.p(d_evk), dbc, self.p(d_y), out_form, self.p(d_work), self.stream), "crc_square_relin_forms")

    def square_pool_relin_supported(self, xf, yf, dbc=16):
        return bool(self.L.crc_square_pool_relin_supported(self.c, dbc, xf, yf))

    def square_pool_relin_work_bytes(self, B, zd, xd, yd, xs, ys, xf, yf, dbc=16):
        return self.L.crc_square_pool_relin_work_bytes(self.c, B, zd, xd, yd, xs, ys, xf, yf, dbc)

    def square_pool_relin(self, d_x, B, zd, xd, yd, xs, ys, xf, yf, d_evk, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF, d_div=None):
        """Square + relinearise + sum / average pooling with one key switch per pooled ciphertext (crc_square_pool_relin_forms)"""
        _chk(self.L.crc_square_pool_relin_forms(self.c, self.p(d_x), in_form, B, zd, xd, yd, xs, ys, xf, yf, self.p(d_evk), dbc, self.p(d_div), self.p(d_y), out_form, self.p(d_work),
                                                self.stream),
             "crc_square_pool_relin_forms")

    def encrypt_dev_work_bytes(self, count):
        return self.L.crc_encrypt_dev_work_bytes(self.c, count)

    def encrypt_dev(self, d_pk, d_plain, count, seed, d_ct, d_work):
        _chk(self.L.crc_encrypt_dev(self.c, self.p(d_pk), self.p(d_plain), count, seed, self.p(d_ct), self.p(d_work), self.stream), "crc_encrypt_dev")

    def encrypt_dev_forms(self, d_pk, d_plain, count, seed, out_form, d_ct, d_work):
        _chk(self.L.crc_encrypt_dev_forms(self.c, self.p(d_pk), self.p(d_plain), count, seed, out_form, self.p(d_ct), self.p(d_work), self.stream),
             "crc_encrypt_dev_forms")

    def encrypt_dev_key_forms(self, d_pk, d_plain, count, key, stream_base, out_form, d_ct, d_work):
        _chk(self.L.crc_encrypt_dev_key_forms(self.c, self.p(d_pk), self.p(d_plain), count, self._key(key), stream_base, out_form, self.p(d_ct),
                                              self.p(d_work), self.stream), "crc_encrypt_dev_key_forms")

    # ---- Decryptor::decrypt / FractionalEncoder / the refresh of Network::forward on the device (kernels_decrypt.hip)
    def decrypt_dev_work_bytes(self, count, size=2, in_form=COEFF):
        return self.L.crc_decrypt_dev_work_bytes(self.c, count, size, in_form)

    def decrypt_dev(self, d_sk, d_ct, count, d_plain, d_work, size=2, in_form=COEFF):
        _chk(self.L.crc_decrypt_dev(self.c, self.p(d_sk), self.p(d_ct), count, size, in_form, self.p(d_plain), self.p(d_work), self.stream), "crc_decrypt_dev")

    # ---- Decryptor::invariant_noise_budget of whole tensors (kernels_budget.hip)
    def noise_budget_dev_work_bytes(self, count, size=2, in_form=COEFF):
        return self.L.crc_noise_budget_dev_work_bytes(self.c, count, size, in_form)

    def noise_budget_dev(self, d_sk, d_ct, count, d_bits, d_work, size=2, in_form=COEFF, d_min=None):
        """d_bits: int32 [count]; d_min (optional): int32 [2] = {smallest budget, index of its first occurrence}"""
        _chk(self.L.crc_noise_budget_dev(self.c, self.p(d_sk), self.p(d_ct), count, size, in_form, self.p(d_bits), self.p(d_min), self.p(d_work), self.stream),
             "crc_noise_budget_dev")

    def budget_bits_host(self, v):
        """v: [..., k, n] coefficient-form residues of c0 + c1 s; the budgets the device routine gives for them, computed on the host (no GPU needed)"""
        v = np.ascontiguousarray(v, dtype=np.uint64)
        lead = v.shape[:-2]
        cnt = int(np.prod(lead)) if lead else 1
        out = np.zeros(cnt, dtype=np.int32)
        _chk(self.L.crc_budget_bits_host(self.c, _pu(v), cnt, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "crc_budget_bits_host")
        return out.reshape(lead) if lead else int(out[0])

    def decode_dev(self, d_plain, count, d_out):
        _chk(self.L.crc_decode_dev(self.c, self.p(d_plain), count, self.p(d_out), self.stream), "crc_decode_dev")

    # ---- degree-2 polynomial activation c2 x^2 + c1 x + c0 (crc_poly2_relin_forms / crc_poly2_pool_relin_forms)
    def poly2_rows(self, c2, c1, c0, window=1, d_div=None):
        """the three NTT-form plaintext rows [k][n] the poly2 calls take, None where a term is absent (c2 == 1, c1 == 0, c0 == 0): encode(c2) and encode(c1) as
        crc_plain_to_ntt leaves them, encode(c0) in delta form.  For the pooled call the window count `window` (xf * yf) is folded into the constant term and an average
        pooling's divisor `d_div` (NTT-form row) into all three -- exact ring arithmetic, done once"""
        c2, c1, c0 = (float(np.float32(v)) for v in (c2, c1, c0))
        if not all(np.isfinite(v) for v in (c2, c1, c0)) or c2 == 0.0:
            raise ValueError("poly2_rows: c2 must be non-zero and every coefficient finite")
        rowb = self.k * self.n * 8

        def row(value, delta):
            plain, _ = self.encode(np.array([value], dtype=np.float32))
            d_plain = self.upload(plain); d_row = self.alloc(rowb)
            if delta:
                self.plain_to_delta(d_plain, 1, NTT, d_row)
            else:
                self.plain_to_ntt(d_plain, 1, d_row)
            if d_div is not None:
                self.multiply_plain_ntt(d_row, d_div, 1, 1, size=1)
            self.sync()
            return d_row
        if c2 != 1.0:
            d_p2 = row(c2, False)
        elif d_div is not None:
            d_p2 = self.alloc(rowb); self.copy_d2d(d_p2, d_div, rowb)
        else:
            d_p2 = None
        d_p1 = row(c1, False) if c1 != 0.0 else None
        d_p0 = None
        if c0 != 0.0:
            plain, _ = self.encode(np.array([c0], dtype=np.float32))
            d_one = self.alloc(rowb); self.plain_to_delta(self.upload(plain), 1, NTT, d_one)
            d_p0 = self.alloc(rowb); self.copy_d2d(d_p0, d_one, rowb)
            for _ in range(int(window) - 1):
                self.add(d_p0, d_one, 1, size=1)
            if d_div is not None:
                self.multiply_plain_ntt(d_p0, d_div, 1, 1, size=1)
            self.sync()
        return d_p2, d_p1, d_p0

    def copy_d2d(self, d_dst, d_src, nbytes):
        _chk(self.L.crc_memcpy_d2d(self.c, self.p(d_dst), self.p(d_src), nbytes, self.stream), "crc_memcpy_d2d")

    def poly2_relin_work_bytes(self, count, dbc=16):
        return self.L.crc_poly2_relin_work_bytes(self.c, count, dbc)

    def poly2_relin(self, d_x, count, d_evk, d_p2, d_p1, d_p0, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """c2 x^2 + c1 x + c0 on `count` ciphertexts with one key switch each; d_p2 / d_p1 / d_p0: poly2_rows (None = 1 / 0 / 0)"""
        _chk(self.L.crc_poly2_relin_forms(self.c, self.p(d_x), in_form, count, self.p(d_evk), dbc, self.p(d_p2), self.p(d_p1), self.p(d_p0), self.p(d_y), out_form,
                                          self.p(d_work), self.stream), "crc_poly2_relin_forms")

    # ---- Galois automorphisms: rotations between the slots of a batched ciphertext (crc_galois_* / crc_apply_galois_forms / crc_rotate_* / crc_sum_slots_forms).
    # A key set is (elts, blobs): the host list of elements and one key blob [crc_evk_words] per element in the same order, on the host or on the device
    def galois_elt_valid(self, g):
        return bool(self.L.crc_galois_elt_valid(self.c, int(g)))

    def galois_elt_rows(self, steps):
        """the element of rotate_rows(steps); 0 for |steps| >= n/2"""
        return int(self.L.crc_galois_elt_rows(self.c, int(steps)))

    def galois_elt_columns(self):
        return int(self.L.crc_galois_elt_columns(self.c))

    def galois_default_elts(self):
        """the elements of KeyGenerator::generate_galois_keys(dbc): 2n - 1, then 3^(2^i), 3^(-2^i) mod 2n"""
        out = np.zeros(_chk(self.L.crc_galois_default_elts(self.c, None, 0), "crc_galois_default_elts"), dtype=np.uint64)
        _chk(self.L.crc_galois_default_elts(self.c, _pu(out), out.size), "crc_galois_default_elts")
        return out

    @staticmethod
    def _elts(elts):
        return np.ascontiguousarray(np.asarray(elts, dtype=np.uint64).reshape(-1))

    def gen_galois_keys(self, seed, sk, dbc=16, elts=None, key=None):
        """-> (elts, blobs [n_elts][crc_evk_words]); elts None: the default set.  With `key`: crc_gen_galois_keys_key"""
        elts = self.galois_default_elts() if elts is None else self._elts(elts)
        gk = np.zeros((elts.size, self.L.crc_evk_words(self.c, dbc)), dtype=np.uint64)
        if key is None:
            _chk(self.L.crc_gen_galois_keys(self.c, seed, _pu(sk), dbc, _pu(elts), elts.size, _pu(gk)), "crc_gen_galois_keys")
        else:
            _chk(self.L.crc_gen_galois_keys_key(self.c, self._key(key), _pu(sk), dbc, _pu(elts), elts.size, _pu(gk)), "crc_gen_galois_keys_key")
        return elts, gk

    def galois_plan(self, g, elts):
        """the indices into elts that apply_galois(g) applies, in order (CrcError where a key is missing)"""
        elts = self._elts(elts); out = (CI * 64)()
        cnt = _chk(self.L.crc_galois_plan(self.c, int(g), _pu(elts), elts.size, out, 64), "crc_galois_plan")
        return [int(out[i]) for i in range(cnt)]

    def galois_permute_dev(self, d_x, count, g, d_x3, accumulate=False):
        _chk(self.L.crc_galois_permute_dev(self.c, self.p(d_x), count, int(g), 1 if accumulate else 0, self.p(d_x3), self.stream), "crc_galois_permute_dev")

    def apply_galois_work_bytes(self, count, dbc=16):
        return self.L.crc_apply_galois_work_bytes(self.c, count, dbc)

    def apply_galois(self, d_x, count, g, d_gk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        elts = self._elts(elts)
        _chk(self.L.crc_apply_galois_forms(self.c, self.p(d_x), in_form, count, int(g), self.p(d_gk), _pu(elts), elts.size, dbc, self.p(d_y), out_form,
                                           self.p(d_work), self.stream), "crc_apply_galois_forms")

    def rotate_rows(self, d_x, count, steps, d_gk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """new slot i of each half = old slot (i + steps) mod n/2; d_work: apply_galois_work_bytes (rotate_columns too)"""
        elts = self._elts(elts)
        _chk(self.L.crc_rotate_rows_forms(self.c, self.p(d_x), in_form, count, int(steps), self.p(d_gk), _pu(elts), elts.size, dbc, self.p(d_y), out_form,
                                          self.p(d_work), self.stream), "crc_rotate_rows_forms")

    def rotate_columns(self, d_x, count, d_gk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        elts = self._elts(elts)
        _chk(self.L.crc_rotate_columns_forms(self.c, self.p(d_x), in_form, count, self.p(d_gk), _pu(elts), elts.size, dbc, self.p(d_y), out_form, self.p(d_work),
                                             self.stream), "crc_rotate_columns_forms")

    def sum_slots_work_bytes(self, count, dbc=16):
        return self.L.crc_sum_slots_work_bytes(self.c, count, dbc)

    def sum_slots(self, d_x, count, d_gk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """every slot of the result = the sum of all n slots mod t (log2 n key switches)"""
        elts = self._elts(elts)
        _chk(self.L.crc_sum_slots_forms(self.c, self.p(d_x), in_form, count, self.p(d_gk), _pu(elts), elts.size, dbc, self.p(d_y), out_form, self.p(d_work),
                                        self.stream), "crc_sum_slots_forms")

    # ---- hoisted rotations and the diagonal product over slots (crc_galois_conjugate_keys* / crc_rotate_hoisted_forms / crc_diag_mac_forms).  Their key set is
    # (elts, CONJUGATED blobs): galois_conjugate_keys of an ordinary set.  An ordinary set passed by mistake cannot be detected and gives garbage
    def galois_ntt_table(self, g):
        """table with NTT(sigma_g(p))[i] = NTT(p)[table[i]] for every modulus"""
        out = np.zeros(self.n, dtype=np.uint32)
        _chk(self.L.crc_galois_ntt_table(self.c, int(g), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "crc_galois_ntt_table")
        return out

    def galois_conjugate_keys(self, elts, gk, dbc=16):
        """host blobs [n_elts][crc_evk_words] -> the conjugated blobs K'_g = sigma_g^-1(K_g), same shape"""
        elts = self._elts(elts)
        gk = np.ascontiguousarray(gk, dtype=np.uint64).reshape(elts.size, self.L.crc_evk_words(self.c, dbc))
        out = np.zeros_like(gk)
        _chk(self.L.crc_galois_conjugate_keys(self.c, _pu(elts), elts.size, dbc, _pu(gk), _pu(out)), "crc_galois_conjugate_keys")
        return out

    def galois_conjugate_keys_dev(self, elts, d_gk, d_out, dbc=16):
        elts = self._elts(elts)
        _chk(self.L.crc_galois_conjugate_keys_dev(self.c, _pu(elts), elts.size, dbc, self.p(d_gk), self.p(d_out), self.stream), "crc_galois_conjugate_keys_dev")

    # ---- seeded key-switching keys (crc_gen_keys_seeded* / crc_seeded_keys_expand*): a key set is (ids, dbc, PUBLIC seed, first rows [n_ids][P][k][n]); id 0 is
    # the evaluation key, every other id a Galois element.  Expanded, a key is an ordinary blob
    def seeded_key_words(self, dbc=16):
        return self.L.crc_seeded_key_words(self.c, dbc)

    def gen_keys_seeded(self, seed, sk, ids, dbc=16, key=None, public_seed=None):
        """-> (first rows [n_ids][crc_seeded_key_words], public seed).  With `key` (PRIVATE) and `public_seed`: crc_gen_keys_seeded_key"""
        ids = self._elts(ids)
        first = np.zeros((ids.size, self.seeded_key_words(dbc)), dtype=np.uint64)
        if key is None:
            _chk(self.L.crc_gen_keys_seeded(self.c, seed, _pu(sk), dbc, _pu(ids), ids.size, _pu(first)), "crc_gen_keys_seeded")
            return first, self.seeded_public_seed(seed)
        _chk(self.L.crc_gen_keys_seeded_key(self.c, self._key(key), self._key(public_seed), _pu(sk), dbc, _pu(ids), ids.size, _pu(first)), "crc_gen_keys_seeded_key")
        return first, bytes(public_seed)

    def seeded_keys_expand(self, first, ids, public_seed, dbc=16, conjugate=False):
        """the host twin of seeded_keys_expand_dev: first rows -> blobs [n_ids][crc_evk_words] (conjugate: the blobs of galois_conjugate_keys)"""
        ids = self._elts(ids)
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(ids.size, self.seeded_key_words(dbc))
        out = np.zeros((ids.size, self.L.crc_evk_words(self.c, dbc)), dtype=np.uint64)
        _chk(self.L.crc_seeded_keys_expand(self.c, _pu(first), _pu(ids), ids.size, dbc, self._key(public_seed), 1 if conjugate else 0, _pu(out)),
             "crc_seeded_keys_expand")
        return out

    def gen_keys_seeded_dev(self, seed, d_sk, ids, d_first, dbc=16, key=None, public_seed=None):
        """secret key [k][n] on the device -> first rows on the device, the bits of gen_keys_seeded; asynchronous, no work buffer -> public seed"""
        ids = self._elts(ids)
        if key is None:
            _chk(self.L.crc_gen_keys_seeded_dev(self.c, seed, self.p(d_sk), dbc, _pu(ids), ids.size, self.p(d_first), self.stream), "crc_gen_keys_seeded_dev")
            return self.seeded_public_seed(seed)
        _chk(self.L.crc_gen_keys_seeded_dev_key(self.c, self._key(key), self._key(public_seed), self.p(d_sk), dbc, _pu(ids), ids.size, self.p(d_first),
                                                self.stream), "crc_gen_keys_seeded_dev_key")
        return bytes(public_seed)

    def seeded_keys_expand_dev(self, d_first, ids, public_seed, d_out, dbc=16, conjugate=False):
        ids = self._elts(ids)
        _chk(self.L.crc_seeded_keys_expand_dev(self.c, self.p(d_first), _pu(ids), ids.size, dbc, self._key(public_seed), 1 if conjugate else 0, self.p(d_out),
                                               self.stream), "crc_seeded_keys_expand_dev")

    def seeded_keys_bytes(self, n_ids, dbc=16):
        return self.L.crc_seeded_keys_bytes(self.c, dbc, n_ids)

    def seeded_keys_save(self, first, ids, public_seed, dbc=16):
        ids = self._elts(ids)
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(ids.size, self.seeded_key_words(dbc))
        buf = np.zeros(self.seeded_keys_bytes(ids.size, dbc), dtype=np.uint8); w = SZ(0)
        _chk(self.L.crc_seeded_keys_save(self.c, _pu(first), _pu(ids), ids.size, dbc, self._key(public_seed), buf.ctypes.data, buf.nbytes, ctypes.byref(w)),
             "crc_seeded_keys_save")
        return buf[:w.value].tobytes()

    def seeded_keys_load(self, blob):
        """-> (first rows [n_ids][crc_seeded_key_words], ids, dbc, public seed)"""
        raw = np.frombuffer(bytes(blob), dtype=np.uint8)
        cnt, dbc = CI(0), CI(0)
        _chk(self.L.crc_seeded_keys_load(self.c, raw.ctypes.data, raw.nbytes, None, None, 0, ctypes.byref(cnt), ctypes.byref(dbc), None), "crc_seeded_keys_load")
        first = np.zeros((cnt.value, self.seeded_key_words(dbc.value)), dtype=np.uint64); ids = np.zeros(cnt.value, dtype=np.uint64)
        sd = (ctypes.c_uint8 * 32)()
        _chk(self.L.crc_seeded_keys_load(self.c, raw.ctypes.data, raw.nbytes, _pu(first), _pu(ids), cnt.value, ctypes.byref(cnt), ctypes.byref(dbc), sd),
             "crc_seeded_keys_load")
        return first, ids, dbc.value, bytes(sd)

    def galois_permute_ntt_dev(self, d_in, rows, g, d_out):
        """NTT-form rows [rows][k][n] -> NTT(sigma_g(INTT(rows)))"""
        _chk(self.L.crc_galois_permute_ntt_dev(self.c, self.p(d_in), rows, int(g), self.p(d_out), self.stream), "crc_galois_permute_ntt_dev")

    def rotate_hoisted_work_bytes(self, count, R, dbc=16):
        return self.L.crc_rotate_hoisted_work_bytes(self.c, count, R, dbc)

    def rotate_hoisted(self, d_x, count, gs, d_cgk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """d_y [R][count] = H_g(d_x) for every g of gs (g = 1: a copy), all from one digit decomposition; d_cgk: the CONJUGATED keys of elts"""
        elts = self._elts(elts); gs = self._elts(gs)
        _chk(self.L.crc_rotate_hoisted_forms(self.c, self.p(d_x), in_form, count, _pu(gs), gs.size, self.p(d_cgk), _pu(elts), elts.size, dbc, self.p(d_y), out_form,
                                             self.p(d_work), self.stream), "crc_rotate_hoisted_forms")

    def diag_mac_work_bytes(self, count, R, dbc=16):
        return self.L.crc_diag_mac_work_bytes(self.c, count, R, dbc)

    def diag_mac(self, d_x, count, gs, d_p_ntt, d_cgk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """d_y [count] = Sum_r P_r (*) H_{gs[r]}(d_x); d_p_ntt [R][k][n]: NTT-form plaintext rows (plain_to_ntt)"""
        elts = self._elts(elts); gs = self._elts(gs)
        _chk(self.L.crc_diag_mac_forms(self.c, self.p(d_x), in_form, count, _pu(gs), gs.size, self.p(d_p_ntt), self.p(d_cgk), _pu(elts), elts.size, dbc, self.p(d_y),
                                       out_form, self.p(d_work), self.stream), "crc_diag_mac_forms")

    def diag_matvec_plan(self, W, M):
        """binding.diag_matvec_plan at this ring: (steps, slot rows [len(steps)][n]) of the non-zero diagonals of W padded to M x M"""
        return diag_matvec_plan(W, M, self.n)

    def bsgs_matvec_plan(self, W, M, B):
        """binding.bsgs_matvec_plan at this ring: (baby_steps, giant_steps, slot rows [giant][baby][n])"""
        return bsgs_matvec_plan(W, M, self.n, B)

    def diag_mac_bsgs_work_bytes(self, count, B, G, dbc=16):
        return self.L.crc_diag_mac_bsgs_work_bytes(self.c, count, B, G, dbc)

    def diag_mac_bsgs(self, d_x, count, gb, gg, d_p_ntt, d_cgk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """d_y [count] = Sum_j H_{gg[j]}( Sum_b P[j][b] (*) H_{gb[b]}(d_x) ); d_p_ntt [G][B][k][n]: NTT-form plaintext rows (plain_to_ntt); B + G key switches"""
        elts = self._elts(elts); gb = self._elts(gb); gg = self._elts(gg)
        _chk(self.L.crc_diag_mac_bsgs_forms(self.c, self.p(d_x), in_form, count, _pu(gb), gb.size, _pu(gg), gg.size, self.p(d_p_ntt), self.p(d_cgk), _pu(elts),
                                            elts.size, dbc, self.p(d_y), out_form, self.p(d_work), self.stream), "crc_diag_mac_bsgs_forms")

    # ---- the packed convolution over slots (crc_conv_slots_*): one channel plane per ciphertext, scalar weights, the conjugated key set of the taps' elements
    def conv_slots_plan(self, M, pitch, H, W, fh, fw, dil=1, pool=1):
        """binding.conv_slots_plan at this ring"""
        return conv_slots_plan(self.n, M, pitch, H, W, fh, fw, dil, pool)

    def conv_slots_pack_weights(self, w):
        """integers of any shape (taken mod t) -> uint64 [k] + shape: the word every position of the constant plaintext's NTT-form row holds, per modulus"""
        w = np.ascontiguousarray(w, dtype=np.int64)
        out = np.zeros((self.k,) + w.shape, dtype=np.uint64)
        _chk(self.L.crc_conv_slots_pack_weights(self.c, w.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), w.size, _pu(out)), "crc_conv_slots_pack_weights")
        return out

    def conv_slots_work_bytes(self, count, Cin, Cout, T, dbc=16):
        return self.L.crc_conv_slots_work_bytes(self.c, count, Cin, Cout, T, dbc)

    def conv_slots(self, d_x, count, Cin, gs, d_w, Cout, d_cgk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """d_y [Cout][count] = Sum_ci Sum_tau w[.][co][ci][tau] H_{gs[tau]}(d_x[ci]); d_x [Cin][count], d_w [k][Cout][Cin][T]: conv_slots_pack_weights"""
        elts = self._elts(elts); gs = self._elts(gs)
        _chk(self.L.crc_conv_slots_forms(self.c, self.p(d_x), in_form, count, Cin, _pu(gs), gs.size, self.p(d_w), Cout, self.p(d_cgk), _pu(elts), elts.size, dbc,
                                         self.p(d_y), out_form, self.p(d_work), self.stream), "crc_conv_slots_forms")

    def conv_slots_plan_geom(self, M, pitch, origin, H, W, fh, fw, dil=1, pad=0, stride=1, pool=1, pool_stride=0):
        """binding.conv_slots_plan_geom at this ring"""
        return conv_slots_plan_geom(self.n, M, pitch, origin, H, W, fh, fw, dil, pad, stride, pool, pool_stride)

    def conv_slots_pack_bias(self, b):
        """integers of any shape (taken mod t) -> uint64 [k] + shape: the word every position of the constant plaintext's NTT-form DELTA row holds
        (plain_to_delta, form = NTT), per modulus"""
        b = np.ascontiguousarray(b, dtype=np.int64)
        out = np.zeros((self.k,) + b.shape, dtype=np.uint64)
        _chk(self.L.crc_conv_slots_pack_bias(self.c, b.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), b.size, _pu(out)), "crc_conv_slots_pack_bias")
        return out

    def conv_slots_bias_mask(self, d_x, count, Cin, gs, d_w, Cout, d_bias, d_mask_ntt, d_cgk, elts, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """conv_slots, then + bias[co] on every slot (d_bias [k][Cout]: conv_slots_pack_bias, or None), then times the plaintext row d_mask_ntt [k][n]
        (plain_to_ntt, or None) -- inside the channel mix's epilogue; bit for bit conv_slots into NTT form, add_plain, multiply_plain_ntt, one inverse transform"""
        elts = self._elts(elts); gs = self._elts(gs)
        _chk(self.L.crc_conv_slots_bias_mask_forms(self.c, self.p(d_x), in_form, count, Cin, _pu(gs), gs.size, self.p(d_w), Cout, self.p(d_bias), self.p(d_mask_ntt),
                                                   self.p(d_cgk), _pu(elts), elts.size, dbc, self.p(d_y), out_form, self.p(d_work), self.stream),
             "crc_conv_slots_bias_mask_forms")

    # ---- the dense layer over channel planes (crc_dense_planes_*): the outputs are rotated, one batched key switch with one key per step
    def dense_planes_plan(self, M, in_slots, out_slots):
        """binding.dense_planes_plan at this ring"""
        return dense_planes_plan(self.n, M, in_slots, out_slots)

    def galois_prepared_key_words(self, dbc=16):
        return self.L.crc_galois_prepared_key_words(self.c, dbc)

    def galois_prepare_keys(self, d_cgk, elts, d_pk=None, dbc=16):
        """the prepared form of the conjugated keys d_cgk of elts, made once: returns d_pk [n_elts][galois_prepared_key_words] (allocated here unless given)"""
        elts = self._elts(elts)
        if d_pk is None:
            d_pk = self.alloc(max(1, elts.size) * self.galois_prepared_key_words(dbc) * 8)
        d_scratch = self.alloc(self.L.crc_evk_words(self.c, dbc) * 8)
        _chk(self.L.crc_galois_prepare_keys_dev(self.c, self.p(d_cgk), _pu(elts), elts.size, dbc, self.p(d_pk), self.p(d_scratch), self.stream),
             "crc_galois_prepare_keys_dev")
        self.sync()                                                    # (the scratch is freed on return)
        return d_pk

    def dense_planes_work_bytes(self, count, Cin, R, dbc=16, prepared=False):
        return self.L.crc_dense_planes_work_bytes(self.c, count, Cin, R, dbc, 1 if prepared else 0)

    def dense_planes(self, d_x, count, Cin, gs, d_p_ntt, d_cgk, elts, d_y, d_work, d_pk=None, dbc=16, in_form=COEFF, out_form=COEFF):
        """d_y [count] = Sum_j H_{gs[j]}( Sum_c P[j][c] (*) d_x[c] ); d_x [Cin][count], d_p_ntt [R][Cin][k][n]: NTT-form plaintext rows (plain_to_ntt); d_pk:
        galois_prepare_keys of (d_cgk, elts), or None -- size d_work with prepared = d_pk is not None"""
        elts = self._elts(elts); gs = self._elts(gs)
        _chk(self.L.crc_dense_planes_forms(self.c, self.p(d_x), in_form, count, Cin, _pu(gs), gs.size, self.p(d_p_ntt), self.p(d_cgk), _pu(elts), elts.size,
                                           self.p(d_pk) if d_pk is not None else None, dbc, self.p(d_y), out_form, self.p(d_work), self.stream), "crc_dense_planes_forms")

    # ---- ciphertext x ciphertext multiply and the degree-3 activation c3 x^3 + c2 x^2 + c1 x + c0 (crc_multiply* / crc_poly3_relin_forms)
    def multiply_relin_work_bytes(self, count, dbc=16):
        return self.L.crc_multiply_relin_work_bytes(self.c, count, dbc)

    def multiply(self, d_x, d_y, count, d_out3, d_work):
        """Evaluator::multiply of `count` pairs of size-2 coefficient-form ciphertexts -> size-3 ciphertexts; d_work: multiply_relin_work_bytes"""
        _chk(self.L.crc_multiply(self.c, self.p(d_x), self.p(d_y), count, self.p(d_out3), self.p(d_work), self.stream), "crc_multiply")

    def multiply_relin(self, d_x, d_y, count, d_evk, d_out, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """relinearize(multiply(x, y)); both inputs in in_form; the result must not overlap an input"""
        _chk(self.L.crc_multiply_relin_forms(self.c, self.p(d_x), self.p(d_y), in_form, count, self.p(d_evk), dbc, self.p(d_out), out_form, self.p(d_work),
                                             self.stream), "crc_multiply_relin_forms")

    def poly3_rows(self, c3, c2, c1, c0):
        """the four NTT-form plaintext rows [k][n] of poly3_relin, None where a term is absent (c3 == 1, c2 == 0, c1 == 0, c0 == 0); c3 == 0 is refused: that
        activation is poly2's"""
        with np.errstate(over="ignore"):                 # (a value beyond float32 becomes inf and is refused below)
            c3, c2, c1, c0 = [float(np.float32(v)) for v in (c3, c2, c1, c0)]
        if not all(np.isfinite(v) for v in (c3, c2, c1, c0)) or c3 == 0.0:
            raise ValueError("poly3_rows: c3 must be non-zero and every coefficient finite")
        rowb = self.k * self.n * 8

        def row(value, delta):
            plain, _ = self.encode(np.array([value], dtype=np.float32))
            d_plain = self.upload(plain); d_row = self.alloc(rowb)
            if delta:
                self.plain_to_delta(d_plain, 1, NTT, d_row)
            else:
                self.plain_to_ntt(d_plain, 1, d_row)
            self.sync()
            return d_row
        return (row(c3, False) if c3 != 1.0 else None, row(c2, False) if c2 != 0.0 else None, row(c1, False) if c1 != 0.0 else None,
                row(c0, True) if c0 != 0.0 else None)

    def poly3_relin_work_bytes(self, count, dbc=16):
        return self.L.crc_poly3_relin_work_bytes(self.c, count, dbc)

    def poly3_relin(self, d_x, count, d_evk, d_p3, d_p2, d_p1, d_p0, d_out, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """c3 x^3 + c2 x^2 + c1 x + c0 on `count` ciphertexts, two key switches each; rows: poly3_rows (None = 1 / 0 / 0 / 0)"""
        _chk(self.L.crc_poly3_relin_forms(self.c, self.p(d_x), in_form, count, self.p(d_evk), dbc, self.p(d_p3), self.p(d_p2), self.p(d_p1), self.p(d_p0),
                                          self.p(d_out), out_form, self.p(d_work), self.stream), "crc_poly3_relin_forms")

    def poly2_pool_relin_supported(self, xf, yf, dbc=16):
        return bool(self.L.crc_poly2_pool_relin_supported(self.c, dbc, xf, yf))

    def poly2_pool_relin_work_bytes(self, B, zd, xd, yd, xs, ys, xf, yf, dbc=16):
        return self.L.crc_poly2_pool_relin_work_bytes(self.c, B, zd, xd, yd, xs, ys, xf, yf, dbc)

    def poly2_pool_relin(self, d_x, B, zd, xd, yd, xs, ys, xf, yf, d_evk, d_p2, d_p1, d_p0, d_y, d_work, dbc=16, in_form=COEFF, out_form=COEFF):
        """the polynomial activation followed by a sum / average pooling, one key switch per pooled ciphertext; the rows carry the window count and the divisor
        (poly2_rows(..., window=xf * yf, d_div=...))"""
        _chk(self.L.crc_poly2_pool_relin_forms(self.c, self.p(d_x), in_form, B, zd, xd, yd, xs, ys, xf, yf, self.p(d_evk), dbc, self.p(d_p2), self.p(d_p1), self.p(d_p0),
                                               self.p(d_y), out_form, self.p(d_work), self.stream), "crc_poly2_pool_relin_forms")

    def encode_dev(self, d_values, count, d_plain, f64=False):
        f = self.L.crc_encode_dev_f64 if f64 else self.L.crc_encode_dev_f32
        _chk(f(self.c, self.p(d_values), count, self.p(d_plain), self.stream), "crc_encode_dev")

    def refresh_dev_work_bytes(self, count, in_form=COEFF):
        return self.L.crc_refresh_dev_work_bytes(self.c, count, in_form)

    def refresh_dev(self, d_sk, d_pk, d_ct_in, count, seed, d_ct_out, d_work, in_form=COEFF, out_form=COEFF, d_values=None, key=None, stream_base=0):
        self._seeded_or_keyed("refresh_dev", (self.c, self.p(d_sk), self.p(d_pk), self.p(d_ct_in), count, in_form), seed, key, stream_base,
                              (out_form, self.p(d_ct_out), self.p(d_values), self.p(d_work), self.stream))

    # ---- encryption under the secret key on the device, and the refresh that uses it
    def seeded_expand_dev(self, d_c0, count, public_seed, stream_base, out_form, d_ct):
        """packed c0 rows [count][k][n] on the device -> ciphertexts [count][2][k][n] in out_form (crc_seeded_expand_dev; asynchronous, no work buffer)"""
        _chk(self.L.crc_seeded_expand_dev(self.c, self.p(d_c0), count, self._key(public_seed), stream_base, out_form, self.p(d_ct), self.stream),
             "crc_seeded_expand_dev")

    def encrypt_sym_seeded_dev(self, d_sk, d_plain, count, seed, d_c0, key=None, public_seed=None, stream_base=0):
        """dense plaintexts [count][n] on the device -> packed c0 rows [count][k][n], the bits of encrypt_sym_seeded (crc_encrypt_sym_seeded_dev; with `key`
        (PRIVATE) and `public_seed`: crc_encrypt_sym_seeded_dev_key).  Asynchronous, no work buffer -> (public seed, stream_base)"""
        if key is None:
            _chk(self.L.crc_encrypt_sym_seeded_dev(self.c, self.p(d_sk), self.p(d_plain), count, seed, self.p(d_c0), self.stream), "crc_encrypt_sym_seeded_dev")
            return self.seeded_public_seed(seed), 0
        _chk(self.L.crc_encrypt_sym_seeded_dev_key(self.c, self.p(d_sk), self.p(d_plain), count, self._key(key), self._key(public_seed), stream_base,
                                                   self.p(d_c0), self.stream), "crc_encrypt_sym_seeded_dev_key")
        return bytes(public_seed), stream_base

    def encrypt_f32_seeded_dev_work_bytes(self, count):
        return self.L.crc_encrypt_f32_seeded_dev_work_bytes(self.c, count)

    def encrypt_f32_seeded_dev(self, d_sk, d_values, count, seed, d_c0, d_work, key=None, public_seed=None, stream_base=0):
        """float32 values [count] on the device -> packed c0 rows: the device encoder in compact form, then the encryptor above (crc_encrypt_f32_seeded_dev[_key])"""
        if key is None:
            _chk(self.L.crc_encrypt_f32_seeded_dev(self.c, self.p(d_sk), self.p(d_values), count, seed, self.p(d_c0), self.p(d_work), self.stream),
                 "crc_encrypt_f32_seeded_dev")
            return self.seeded_public_seed(seed), 0
        _chk(self.L.crc_encrypt_f32_seeded_dev_key(self.c, self.p(d_sk), self.p(d_values), count, self._key(key), self._key(public_seed), stream_base,
                                                   self.p(d_c0), self.p(d_work), self.stream), "crc_encrypt_f32_seeded_dev_key")
        return bytes(public_seed), stream_base

    def encrypt_sym_dev_work_bytes(self, count):
        return self.L.crc_encrypt_sym_dev_work_bytes(self.c, count)

    def encrypt_sym_dev_forms(self, d_sk, d_plain, count, seed, out_form, d_ct, d_work):
        _chk(self.L.crc_encrypt_sym_dev_forms(self.c, self.p(d_sk), self.p(d_plain), count, seed, out_form, self.p(d_ct), self.p(d_work), self.stream),
             "crc_encrypt_sym_dev_forms")

    def encrypt_sym_dev(self, d_sk, d_plain, count, seed, d_ct, d_work):
        self.encrypt_sym_dev_forms(d_sk, d_plain, count, seed, COEFF, d_ct, d_work)

    def encrypt_sym_dev_key_forms(self, d_sk, d_plain, count, key, stream_base, out_form, d_ct, d_work):
        _chk(self.L.crc_encrypt_sym_dev_key_forms(self.c, self.p(d_sk), self.p(d_plain), count, self._key(key), stream_base, out_form, self.p(d_ct),
                                                  self.p(d_work), self.stream), "crc_encrypt_sym_dev_key_forms")

    def encrypt_sym_dev_key(self, d_sk, d_plain, count, key, stream_base, d_ct, d_work):
        self.encrypt_sym_dev_key_forms(d_sk, d_plain, count, key, stream_base, COEFF, d_ct, d_work)

    def refresh_sym_dev_work_bytes(self, count, in_form=COEFF):
        return self.L.crc_refresh_sym_dev_work_bytes(self.c, count, in_form)

    def refresh_sym_dev(self, d_sk, d_ct_in, count, seed, d_ct_out, d_work, in_form=COEFF, out_form=COEFF, d_values=None, key=None, stream_base=0):
        self._seeded_or_keyed("refresh_sym_dev", (self.c, self.p(d_sk), self.p(d_ct_in), count, in_form), seed, key, stream_base,
                              (out_form, self.p(d_ct_out), self.p(d_values), self.p(d_work), self.stream))

    def encrypt_dev_noise_thresholds(self):
        out = (ctypes.c_uint64 * 19)()
        self.L.crc_encrypt_dev_noise_thresholds(out)
        return [int(v) for v in out]

    def encrypt_dev_key(self, d_pk, d_plain, count, key, stream_base, d_ct, d_work):
        _chk(self.L.crc_encrypt_dev_key(self.c, self.p(d_pk), self.p(d_plain), count, self._key(key), stream_base, self.p(d_ct), self.p(d_work), self.stream), "crc_encrypt_dev_key")

    # ---- multi-GPU: RCCL communicator bound to this context's device
    def comm_unique_id(self):
        buf = (ctypes.c_uint8 * 128)()
        _chk(self.L.crc_comm_unique_id(buf), "crc_comm_unique_id"); return bytes(buf)

    def comm_create(self, world, rank, uid):
        assert len(uid) == 128
        out = VP()
        _chk(self.L.crc_comm_create(self.c, world, rank, (ctypes.c_uint8 * 128).from_buffer_copy(bytes(uid)), ctypes.byref(out)), "crc_comm_create")
        return out

    def comm_destroy(self, comm):
        self.L.crc_comm_destroy(comm)

    def broadcast_weights(self, comm, d_w, nbytes, root=0):
        assert nbytes % 8 == 0
        _chk(self.L.crc_broadcast_weights(comm, self.p(d_w), nbytes // 8, root, self.stream), "crc_broadcast_weights")

    def allgather_u64(self, comm, values):
        v = np.ascontiguousarray(values, dtype=np.uint64)
        out = np.zeros((self.L.crc_comm_world(comm), v.size), dtype=np.uint64)
        _chk(self.L.crc_comm_allgather_u64(comm, _pu(v), v.size, _pu(out), self.stream), "crc_comm_allgather_u64")
        return out

    def checksum64(self, d_words, nbytes):
        out = np.zeros(2, dtype=np.uint64)
        _chk(self.L.crc_checksum64(self.c, self.p(d_words), nbytes // 8, _pu(out), self.stream), "crc_checksum64")
        return int(out[0]), int(out[1])

    def square(self, d_x, count, d_y3, d_work):
        _chk(self.L.crc_square(self.c, self.p(d_x), count, self.p(d_y3), self.p(d_work), self.stream), "crc_square")

    def relinearize(self, d_x3, count, d_evk, d_y, d_work, dbc=16):
        _chk(self.L.crc_relinearize(self.c, self.p(d_x3), count, self.p(d_evk), dbc, self.p(d_y), self.p(d_work), self.stream), "crc_relinearize")


class SlotsCrt:
    """A residue base: r <= 4 Engines of one n, q and device whose slot primes t_j are pairwise distinct with T = prod t_j < 2**63 (crc_slots_crt_*).  The same
    network runs under every engine; the slots recombine into centred integers mod T.  Keys do not involve t: one key set serves all engines"""
    MAX = 4

    def __init__(self, engines):
        self.E = list(engines)
        self.L = self.E[0].L
        self.r, self.n = len(self.E), self.E[0].n
        self.ts = [e.t for e in self.E]
        self.T = int(np.prod([int(t) for t in self.ts], dtype=object))
        self.stream = self.E[0].stream

    def _ctxs(self):
        return (VP * self.r)(*[e.c for e in self.E])

    def _rows(self, bufs):
        assert len(bufs) == self.r
        return (VP * self.r)(*[Engine.p(b) for b in bufs])

    @property
    def supported(self):
        return bool(self.L.crc_slots_crt_supported(self._ctxs(), self.r))

    @staticmethod
    def primes(n, r, bits):
        """the r largest primes below 2**bits that are 1 mod 2n, descending"""
        t = np.zeros(r, dtype=np.uint64)
        _chk(load().crc_slots_crt_primes(int(n), int(r), int(bits), _pu(t)), "crc_slots_crt_primes")
        return [int(x) for x in t]

    def compose(self, values, count, slots, item_stride, slot_stride):
        """host: the r existing calls on the same int64 values -> [r][count][n]"""
        return np.stack([e.slots_compose(values, count, slots, item_stride, slot_stride) for e in self.E])

    def compose_dev(self, d_values, count, slots, item_stride, slot_stride, d_plains):
        for e, d in zip(self.E, d_plains):
            e.slots_compose_dev(d_values, count, slots, item_stride, slot_stride, d)

    def decompose(self, plains, slots, item_stride, slot_stride, size=None):
        """host twin: plaintexts [r][count][n] -> flat int64 array, the centred integers mod T"""
        plains = np.ascontiguousarray(plains, dtype=np.uint64).reshape(self.r, -1, self.n); count = plains.shape[1]
        need = (count - 1) * item_stride + (slots - 1) * slot_stride + 1
        out = np.zeros(need if size is None else size, dtype=np.int64)
        assert out.size >= need
        rows = (VP * self.r)(*[plains[j].ctypes.data for j in range(self.r)])
        _chk(self.L.crc_slots_crt_decompose(self._ctxs(), self.r, rows, count, slots, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), item_stride, slot_stride),
             "crc_slots_crt_decompose")
        return out

    def decompose_dev(self, d_plains, count, slots, d_values, item_stride, slot_stride):
        _chk(self.L.crc_slots_crt_decompose_dev(self._ctxs(), self.r, self._rows(d_plains), count, slots, Engine.p(d_values), item_stride, slot_stride, self.stream),
             "crc_slots_crt_decompose_dev")

    def act(self, plains, divisor, relu=0, cap=0):
        """host twin: plaintexts [r][count][n] -> [r][count][n]; per slot floor(V / divisor + 1/2) of the lifted integer V, ReLU, cap, reduced mod every t_j"""
        plains = np.ascontiguousarray(plains, dtype=np.uint64).reshape(self.r, -1, self.n)
        out = np.zeros_like(plains)
        rin = (VP * self.r)(*[plains[j].ctypes.data for j in range(self.r)])
        rout = (VP * self.r)(*[out[j].ctypes.data for j in range(self.r)])
        _chk(self.L.crc_slots_crt_act(self._ctxs(), self.r, rin, plains.shape[1], int(divisor), int(relu), int(cap), rout), "crc_slots_crt_act")
        return out

    def act_dev(self, d_in, count, divisor, relu, cap, d_out):
        _chk(self.L.crc_slots_crt_act_dev(self._ctxs(), self.r, self._rows(d_in), count, int(divisor), int(relu), int(cap), self._rows(d_out), self.stream),
             "crc_slots_crt_act_dev")

    def refresh_dev_work_bytes(self, count, in_form=COEFF):
        return self.L.crc_slots_crt_refresh_dev_work_bytes(self._ctxs(), self.r, count, in_form)

    refresh_sym_dev_work_bytes = refresh_dev_work_bytes           # one size serves either call

    def refresh_dev(self, d_sk, d_pk, d_ct_in, count, divisor, relu, cap, key, stream_base, d_ct_out, d_work, in_form=COEFF, out_form=COEFF):
        """on every engine: decrypt -> the CRT activation over the r plaintext tensors -> encrypt under the public key (stream base stream_base + j * count)"""
        _chk(self.L.crc_slots_crt_refresh_dev_key(self._ctxs(), self.r, Engine.p(d_sk), Engine.p(d_pk), self._rows(d_ct_in), count, in_form, int(divisor), int(relu),
                                                  int(cap), Engine._key(key), stream_base, out_form, self._rows(d_ct_out), Engine.p(d_work), self.stream),
             "crc_slots_crt_refresh_dev_key")

    def refresh_sym_dev(self, d_sk, d_ct_in, count, divisor, relu, cap, key, stream_base, d_ct_out, d_work, in_form=COEFF, out_form=COEFF):
        """the same under the secret key"""
        _chk(self.L.crc_slots_crt_refresh_sym_dev_key(self._ctxs(), self.r, Engine.p(d_sk), self._rows(d_ct_in), count, in_form, int(divisor), int(relu), int(cap),
                                                      Engine._key(key), stream_base, out_form, self._rows(d_ct_out), Engine.p(d_work), self.stream),
             "crc_slots_crt_refresh_sym_dev_key")
