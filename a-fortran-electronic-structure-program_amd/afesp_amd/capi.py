"""ctypes binding of libafesp_hip.so (include/afesp.h).  Python-side mirror of the three calls the reference's driver
makes into the hot path (src/main.F90:98,105,112): `do_mp2_spatial`, `do_ccsd_spatial`, `do_ccsd_t_spatial`.

There is no CPU fallback: if the shared library is missing, or no GPU is visible, this raises.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AFESP_LIBRARY: a differently built libafesp_hip (A/B kernel measurements inside one GPU session, tools/ab_gemm.py)
LIB_PATH = os.environ.get("AFESP_LIBRARY") or os.path.join(os.path.dirname(_HERE), "csrc", "libafesp_hip.so")

i64 = C.c_int64
dbl = C.c_double
_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_opt = C.c_void_p

EXPORTS = [
    "afesp_ctx_create", "afesp_ctx_destroy", "afesp_last_error", "afesp_version", "afesp_neri", "afesp_ao2mo_mp2",
    "afesp_ccsd_init", "afesp_ccsd_iterate", "afesp_ccsd_energy", "afesp_ccsd_diis", "afesp_ccsd_solve",
    "afesp_ccsd_get_amplitudes", "afesp_ccsd_set_amplitudes", "afesp_ccsd_get_tensor", "afesp_ccsd_update_intermediates",
    "afesp_ccsd_update_amplitudes", "afesp_ccsd_t_ntriples", "afesp_ccsd_t", "afesp_ccsd_t_shard_bounds", "afesp_gemm", "afesp_permute4",
    "afesp_contract", "afesp_synthetic_init", "afesp_time_pp_ladder", "afesp_bench_contract", "afesp_set_tuning", "afesp_bench_stream", "afesp_profile", "afesp_ccsd_cr_intermediates", "afesp_ccsd_t_cr",
    "afesp_ccsd_so_init", "afesp_ccsd_so_energy", "afesp_ccsd_so_iterate", "afesp_ccsd_so_diis", "afesp_ccsd_so_get_amplitudes",
    "afesp_ccsd_so_set_amplitudes", "afesp_ccsd_so_get_tensor", "afesp_ccsd_so_t_ntriples", "afesp_ccsd_so_t",
    "afesp_ccsd_so_lambda_init", "afesp_ccsd_so_lambda_iterate", "afesp_ccsd_so_lambda_energy", "afesp_ccsd_so_lambda_diis",
    "afesp_ccsd_so_get_lambda", "afesp_ccsd_so_set_lambda", "afesp_ccsd_so_density", "afesp_ccsd_so_lambda_t",
    "afesp_ccsd_so_eom_t",
    "afesp_ccsd_so_density2_build", "afesp_ccsd_so_density2_get", "afesp_ccsd_so_density2_energy", "afesp_ccsd_so_density2_expect",
    "afesp_ccsd_so_orbital_gradient", "afesp_ccsd_so_zvector_apply", "afesp_ccsd_so_zvector_solve", "afesp_ccsd_so_relaxed_density",
    "afesp_ccsd_so_relax_pair_row",
    "afesp_ccsd_so_eom_init", "afesp_ccsd_so_eom_sigma", "afesp_ccsd_so_eom_guess", "afesp_ccsd_so_eom_set_guess",
    "afesp_ccsd_so_eom_iterate", "afesp_ccsd_so_eom_get_vector", "afesp_eig_general",
    "afesp_ccsd_so_eom_lsigma", "afesp_ccsd_so_eom_left_init", "afesp_ccsd_so_eom_left_guess", "afesp_ccsd_so_eom_left_set_guess",
    "afesp_ccsd_so_eom_left_iterate", "afesp_ccsd_so_eom_left_get_vector", "afesp_ccsd_so_eom_ref_coupling", "afesp_ccsd_so_eom_density",
    "afesp_ccsd_so_eom_ipea_init", "afesp_ccsd_so_eom_ipea_sigma", "afesp_ccsd_so_eom_ipea_guess", "afesp_ccsd_so_eom_ipea_set_guess",
    "afesp_ccsd_so_eom_ipea_iterate", "afesp_ccsd_so_eom_ipea_get_vector",
    "afesp_ccsd_so_eom_ipea_lsigma", "afesp_ccsd_so_eom_ipea_left_init", "afesp_ccsd_so_eom_ipea_left_guess",
    "afesp_ccsd_so_eom_ipea_left_set_guess", "afesp_ccsd_so_eom_ipea_left_iterate", "afesp_ccsd_so_eom_ipea_left_get_vector",
    "afesp_ccsd_so_eom_ipea_dyson", "afesp_ccsd_so_eom_ipea_t", "afesp_ccsd_so_eom_ipea_t_nitems",
    "afesp_ccsd_so_response_xi", "afesp_ccsd_so_response_init", "afesp_ccsd_so_response_iterate", "afesp_ccsd_so_response_get_vector",
    "afesp_ccsd_so_response_function", "afesp_lu_solve",
    "afesp_ccsd_so_response_init_complex", "afesp_ccsd_so_response_get_vector_complex", "afesp_ccsd_so_response_function_complex",
    "afesp_lu_solve_complex",
    "afesp_read_eri_text", "afesp_write_fcidump", "afesp_set_eri", "afesp_build_fock", "afesp_ccsd_t_plain",
    "afesp_synthetic_ao", "afesp_ccsd_pp_ladder_flop", "afesp_ccsd_iteration_flop",
    "afesp_device_count", "afesp_comm_unique_id", "afesp_comm_init", "afesp_comm_destroy", "afesp_allreduce_sum",
    "afesp_build_fock_uhf", "afesp_ao2mo_ump2", "afesp_ccsd_uso_init", "afesp_mo_window", "afesp_umo_window",
    "afesp_mp2_vv_density", "afesp_ump2_vv_density",
    "afesp_core_operator", "afesp_ucore_operator", "afesp_write_fcidump_active", "afesp_write_fcidump_uactive",
    "afesp_fcidump_scan", "afesp_read_fcidump", "afesp_read_fcidump_uhf",
    "afesp_mo_fock_ro", "afesp_read_fcidump_rohf", "afesp_mo_rotate_uhf", "afesp_ccsd_uso_init_fock",
    "afesp_ccsd_t_block_size", "afesp_test_inject", "afesp_ccsd_is_split", "afesp_ccsd_set_split", "afesp_ccsd_set_fused", "afesp_ccsd_iteration_launches", "afesp_debug_stamps", "afesp_launch_counts", "afesp_first_use_count", "afesp_test_ring_path", "afesp_arena_stats",
    "afesp_test_davidson_create", "afesp_test_davidson_destroy", "afesp_test_davidson_set_guess", "afesp_test_davidson_iterate",
    "afesp_test_davidson_linear_start", "afesp_test_davidson_linear_start_complex", "afesp_test_davidson_linear_iterate", "afesp_test_davidson_get_vector", "afesp_test_davidson_fetch",
]
COMM_RCCL, COMM_HOST = 0, 1


class AfespError(RuntimeError):
    pass


_lib = None


def load_library():
    """dlopen the HIP library.  Raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AfespError(f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}` "
                         "(there is no CPU fallback for the accelerated path)")
    L = C.CDLL(LIB_PATH)
    L.afesp_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.afesp_ctx_destroy.argtypes = [C.c_void_p]
    L.afesp_ctx_destroy.restype = None
    L.afesp_last_error.argtypes = [C.c_void_p]
    L.afesp_last_error.restype = C.c_char_p
    L.afesp_neri.argtypes = [i64]
    L.afesp_neri.restype = i64
    L.afesp_ao2mo_mp2.argtypes = [C.c_void_p, i64, i64, _dp, _dp, _opt, _opt, C.POINTER(dbl)]
    L.afesp_ccsd_init.argtypes = [C.c_void_p, i64, i64, _opt, _dp, C.c_int]
    L.afesp_ccsd_iterate.argtypes = [C.c_void_p, dbl, dbl, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int)]
    L.afesp_ccsd_energy.argtypes = [C.c_void_p, dbl, dbl, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int)]
    L.afesp_ccsd_diis.argtypes = [C.c_void_p]
    L.afesp_ccsd_solve.argtypes = [C.c_void_p, C.c_int, dbl, dbl, _dp, _dp, C.POINTER(C.c_int)]
    L.afesp_ccsd_get_amplitudes.argtypes = [C.c_void_p, _dp, _dp]
    L.afesp_ccsd_set_amplitudes.argtypes = [C.c_void_p, _dp, _dp]
    L.afesp_ccsd_get_tensor.argtypes = [C.c_void_p, C.c_char_p, _dp, i64]
    L.afesp_ccsd_update_intermediates.argtypes = [C.c_void_p]
    L.afesp_ccsd_update_amplitudes.argtypes = [C.c_void_p]
    L.afesp_ccsd_t_ntriples.argtypes = [i64]
    L.afesp_ccsd_t_ntriples.restype = i64
    L.afesp_ccsd_t_shard_bounds.argtypes = [C.c_void_p, i64, i64, C.c_int, C.c_int, C.POINTER(i64)]
    L.afesp_ccsd_t.argtypes = [C.c_void_p, i64, i64, _dp]
    L.afesp_ccsd_t_cr.argtypes = [C.c_void_p, i64, i64, _dp]
    L.afesp_ccsd_t_plain.argtypes = [C.c_void_p, i64, i64, _dp]
    L.afesp_ccsd_cr_intermediates.argtypes = [C.c_void_p]
    L.afesp_gemm.argtypes = [C.c_void_p, C.c_char, C.c_char, i64, i64, i64, dbl, _dp, _dp, dbl, _dp]
    L.afesp_permute4.argtypes = [C.c_void_p, C.POINTER(i64), C.c_char_p, _dp, _dp, C.c_int, dbl]
    L.afesp_contract.argtypes = [C.c_void_p, dbl, _dp, C.c_char_p, C.POINTER(i64), _dp, C.c_char_p, C.POINTER(i64), dbl,
                                 _dp, C.c_char_p, C.POINTER(i64), C.c_int, C.c_int, C.c_int]
    L.afesp_synthetic_init.argtypes = [C.c_void_p, i64, i64, dbl, C.c_uint64, C.c_int]
    L.afesp_time_pp_ladder.argtypes = [C.c_void_p, C.c_int, C.POINTER(dbl)]
    L.afesp_synthetic_ao.argtypes = [C.c_void_p, i64, dbl, C.c_uint64]
    L.afesp_ccsd_pp_ladder_flop.argtypes = [C.c_void_p, C.POINTER(dbl)]
    L.afesp_ccsd_iteration_flop.argtypes = [C.c_void_p, C.POINTER(dbl)]
    L.afesp_bench_contract.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(i64), C.c_char_p, C.POINTER(i64), C.c_char_p,
                                       C.POINTER(i64), C.c_int, C.POINTER(dbl)]
    L.afesp_set_tuning.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.afesp_bench_stream.argtypes = [C.c_void_p, i64, C.c_int, C.POINTER(dbl)]
    L.afesp_profile.argtypes = [C.c_void_p, C.c_int, _dp]
    L.afesp_ccsd_so_init.argtypes = [C.c_void_p, i64, i64, _opt, _dp, C.c_int, C.c_int]
    L.afesp_ccsd_so_iterate.argtypes = [C.c_void_p, dbl, dbl, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_energy.argtypes = [C.c_void_p, dbl, dbl, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_diis.argtypes = [C.c_void_p]
    L.afesp_ccsd_so_get_amplitudes.argtypes = [C.c_void_p, _dp, _dp]
    L.afesp_ccsd_so_set_amplitudes.argtypes = [C.c_void_p, _dp, _dp]
    L.afesp_ccsd_so_get_tensor.argtypes = [C.c_void_p, C.c_char_p, _dp, i64]
    L.afesp_ccsd_so_t_ntriples.argtypes = [i64]
    L.afesp_ccsd_so_t_ntriples.restype = i64
    L.afesp_ccsd_so_t.argtypes = [C.c_void_p, i64, i64, C.POINTER(dbl)]
    L.afesp_ccsd_so_lambda_init.argtypes = [C.c_void_p, C.c_int]
    L.afesp_ccsd_so_lambda_iterate.argtypes = [C.c_void_p, dbl, dbl, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_lambda_energy.argtypes = [C.c_void_p, dbl, dbl, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_lambda_diis.argtypes = [C.c_void_p]
    L.afesp_ccsd_so_get_lambda.argtypes = [C.c_void_p, _dp, _dp]
    L.afesp_ccsd_so_set_lambda.argtypes = [C.c_void_p, _dp, _dp]
    L.afesp_ccsd_so_density.argtypes = [C.c_void_p, _dp, i64]
    L.afesp_ccsd_so_lambda_t.argtypes = [C.c_void_p, i64, i64, C.POINTER(dbl)]
    L.afesp_ccsd_so_eom_t.argtypes = [C.c_void_p, C.c_int, _opt, _opt, _opt, _opt, _opt, i64, i64, _opt]
    L.afesp_ccsd_so_density2_build.argtypes = [C.c_void_p]
    L.afesp_ccsd_so_density2_get.argtypes = [C.c_void_p, C.c_char_p, _opt, i64]
    L.afesp_ccsd_so_density2_energy.argtypes = [C.c_void_p, _opt]
    L.afesp_ccsd_so_density2_expect.argtypes = [C.c_void_p, _opt, _opt, _opt]
    L.afesp_ccsd_so_orbital_gradient.argtypes = [C.c_void_p, C.c_int, _opt, i64]
    L.afesp_ccsd_so_zvector_apply.argtypes = [C.c_void_p, _opt, _opt]
    L.afesp_ccsd_so_zvector_solve.argtypes = [C.c_void_p, dbl, C.c_int, _opt, C.POINTER(C.c_int), C.POINTER(dbl)]
    L.afesp_ccsd_so_relaxed_density.argtypes = [C.c_void_p, _opt, i64]
    L.afesp_ccsd_so_relax_pair_row.argtypes = [C.c_void_p, C.c_int, _opt, C.c_int, C.POINTER(dbl)]
    L.afesp_ccsd_so_eom_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.afesp_ccsd_so_eom_sigma.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    L.afesp_ccsd_so_eom_guess.argtypes = [C.c_void_p]
    L.afesp_ccsd_so_eom_set_guess.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_ccsd_so_eom_iterate.argtypes = [C.c_void_p, dbl, _dp, _dp, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS"),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_eom_get_vector.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_ccsd_so_eom_lsigma.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    L.afesp_ccsd_so_eom_left_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.afesp_ccsd_so_eom_left_guess.argtypes = [C.c_void_p]
    L.afesp_ccsd_so_eom_left_set_guess.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_ccsd_so_eom_left_iterate.argtypes = [C.c_void_p, dbl, _dp, _dp, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS"),
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_eom_left_get_vector.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_ccsd_so_eom_ref_coupling.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    L.afesp_ccsd_so_eom_density.argtypes = [C.c_void_p, dbl, _opt, _opt, dbl, _opt, _opt, _dp, i64]
    L.afesp_ccsd_so_response_xi.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    L.afesp_ccsd_so_response_init.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int, _dp, C.c_int]
    L.afesp_ccsd_so_response_iterate.argtypes = [C.c_void_p, dbl, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_response_get_vector.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
    L.afesp_ccsd_so_response_function.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_lu_solve.argtypes = [C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, dbl]
    L.afesp_ccsd_so_response_init_complex.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int, _dp, C.c_int]
    L.afesp_ccsd_so_response_get_vector_complex.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp]
    L.afesp_ccsd_so_response_function_complex.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_lu_solve_complex.argtypes = [C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, dbl]
    L.afesp_ccsd_so_eom_ipea_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.afesp_ccsd_so_eom_ipea_sigma.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp]
    L.afesp_ccsd_so_eom_ipea_guess.argtypes = [C.c_void_p, C.c_int]
    L.afesp_ccsd_so_eom_ipea_set_guess.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
    L.afesp_ccsd_so_eom_ipea_iterate.argtypes = [C.c_void_p, C.c_int, dbl, _dp, _dp, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS"),
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.afesp_ccsd_so_eom_ipea_get_vector.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
    L.afesp_ccsd_so_eom_ipea_lsigma.argtypes = L.afesp_ccsd_so_eom_ipea_sigma.argtypes
    L.afesp_ccsd_so_eom_ipea_left_init.argtypes = L.afesp_ccsd_so_eom_ipea_init.argtypes
    L.afesp_ccsd_so_eom_ipea_left_guess.argtypes = L.afesp_ccsd_so_eom_ipea_guess.argtypes
    L.afesp_ccsd_so_eom_ipea_left_set_guess.argtypes = L.afesp_ccsd_so_eom_ipea_set_guess.argtypes
    L.afesp_ccsd_so_eom_ipea_left_iterate.argtypes = L.afesp_ccsd_so_eom_ipea_iterate.argtypes
    L.afesp_ccsd_so_eom_ipea_left_get_vector.argtypes = L.afesp_ccsd_so_eom_ipea_get_vector.argtypes
    L.afesp_ccsd_so_eom_ipea_dyson.argtypes = [C.c_void_p, C.c_int, C.c_int, _opt, _opt, _opt, _opt, _opt, _opt]
    L.afesp_ccsd_so_eom_ipea_t.argtypes = [C.c_void_p, C.c_int, C.c_int, _opt, _opt, _opt, _opt, _opt, i64, i64, _opt]
    L.afesp_ccsd_so_eom_ipea_t_nitems.argtypes = [C.c_int, C.c_int]
    L.afesp_ccsd_so_eom_ipea_t_nitems.restype = i64
    L.afesp_eig_general.argtypes = [C.c_int, _dp, C.c_int, _dp, _dp, _dp]
    L.afesp_read_eri_text.argtypes = [C.c_void_p, C.c_char_p, i64, _opt, C.POINTER(i64)]
    L.afesp_write_fcidump.argtypes = [C.c_void_p, C.c_char_p, i64, C.POINTER(i64)]
    L.afesp_set_eri.argtypes = [C.c_void_p, i64, _dp]
    L.afesp_build_fock.argtypes = [C.c_void_p, i64, _dp, _dp, _dp]
    L.afesp_build_fock_uhf.argtypes = [C.c_void_p, i64, _dp, _dp, _dp, _dp, _dp]
    L.afesp_ao2mo_ump2.argtypes = [C.c_void_p, i64, i64, i64, _dp, _dp, _dp, _dp, _opt, _opt, _opt, _opt, C.POINTER(dbl)]
    L.afesp_ccsd_uso_init.argtypes = [C.c_void_p, i64, i64, i64, _dp, _dp, C.c_int]
    L.afesp_mo_window.argtypes = [C.c_void_p, i64, i64, i64, i64, _dp, _opt, _opt, C.POINTER(dbl)]
    L.afesp_umo_window.argtypes = [C.c_void_p, i64, i64, i64, i64, i64, _dp, _dp, _opt, _opt, _opt, C.POINTER(dbl)]
    L.afesp_mp2_vv_density.argtypes = [C.c_void_p, i64, i64, i64, _dp, _dp, C.POINTER(dbl)]
    L.afesp_ump2_vv_density.argtypes = [C.c_void_p, i64, i64, i64, i64, _dp, _dp, _dp, _dp, C.POINTER(dbl)]
    L.afesp_core_operator.argtypes = [C.c_void_p, i64, i64, i64, _dp, _dp, _dp, C.POINTER(dbl)]
    L.afesp_ucore_operator.argtypes = [C.c_void_p, i64, i64, i64, _dp, _dp, _dp, _dp, _dp, C.POINTER(dbl)]
    L.afesp_write_fcidump_active.argtypes = [C.c_void_p, C.c_char_p, i64, i64, i64, _dp, dbl, dbl, C.POINTER(i64)]
    L.afesp_write_fcidump_uactive.argtypes = [C.c_void_p, C.c_char_p, i64, i64, i64, _dp, _dp, dbl, dbl, C.POINTER(i64)]
    L.afesp_fcidump_scan.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int), C.POINTER(i64)]
    L.afesp_read_fcidump.argtypes = [C.c_void_p, C.c_char_p, i64, i64, _opt, _opt, _opt, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), _opt,
                                     C.POINTER(i64)]
    L.afesp_read_fcidump_uhf.argtypes = [C.c_void_p, C.c_char_p, i64, i64, i64] + [_opt] * 6 + [C.POINTER(dbl)] * 3 + [_opt] * 3 + [C.POINTER(i64)]
    L.afesp_mo_fock_ro.argtypes = [C.c_void_p, i64, i64, i64, _dp, _dp, _dp, C.POINTER(dbl)]
    L.afesp_read_fcidump_rohf.argtypes = [C.c_void_p, C.c_char_p, i64, i64, i64, _opt, _opt, _opt, C.POINTER(dbl), C.POINTER(dbl), _opt, _opt,
                                          C.POINTER(i64)]
    L.afesp_mo_rotate_uhf.argtypes = [C.c_void_p, i64, _dp, _dp, _opt, _opt, _opt]
    L.afesp_ccsd_uso_init_fock.argtypes = [C.c_void_p, i64, i64, i64, _dp, _dp, C.c_int, C.POINTER(dbl)]
    L.afesp_device_count.argtypes = []
    L.afesp_comm_unique_id.argtypes = [C.c_char_p]
    L.afesp_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
    L.afesp_comm_destroy.argtypes = [C.c_void_p]
    L.afesp_allreduce_sum.argtypes = [C.c_void_p, _dp, i64]
    L.afesp_ccsd_t_block_size.argtypes = [C.c_void_p, i64, i64, C.c_int, C.POINTER(C.c_int)]
    L.afesp_test_inject.argtypes = [C.c_void_p, C.c_int]
    L.afesp_arena_stats.argtypes = [C.c_void_p, _dp]
    L.afesp_ccsd_is_split.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.afesp_ccsd_set_split.argtypes = [C.c_void_p, C.c_int]
    L.afesp_ccsd_set_fused.argtypes = [C.c_void_p, C.c_int]
    L.afesp_ccsd_iteration_launches.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.afesp_debug_stamps.argtypes = [C.c_void_p, C.c_int]
    L.afesp_launch_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.afesp_first_use_count.argtypes = []
    L.afesp_first_use_count.restype = C.c_uint64
    L.afesp_test_ring_path.argtypes = [C.c_int64, C.c_int64]
    _ip = C.POINTER(C.c_int)
    L.afesp_test_davidson_create.argtypes = [C.c_void_p, i64, i64, dbl, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp]
    L.afesp_test_davidson_destroy.argtypes = [C.c_void_p]
    L.afesp_test_davidson_set_guess.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_test_davidson_iterate.argtypes = [C.c_void_p, dbl, _dp, _dp, _ip, _ip, _ip]
    L.afesp_test_davidson_linear_start.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_test_davidson_linear_start_complex.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp]
    L.afesp_test_davidson_linear_iterate.argtypes = [C.c_void_p, dbl, _dp, _ip, _ip, _ip]
    L.afesp_test_davidson_get_vector.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.afesp_test_davidson_fetch.argtypes = [C.c_void_p, C.c_char_p, _dp, i64, C.POINTER(i64)]
    _lib = L
    return L


def _f(a):
    """Fortran-order flat copy of an array (what the C-ABI expects)."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel(order="F"))


TENSOR_SHAPES = {
    "v_oovv": "oovv", "v_ovov": "ovov", "v_vvov": "vvov", "v_oovo": "oovo", "v_oooo": "oooo", "v_vvvv": "vvvv",
    "I_vo": "vo", "I_vv": "vv", "I_oo_p": "oo", "I_oo": "oo", "c_oovv": "oovv", "asym_t2": "oovv", "x_voov": "voov",
    "I_oooo": "oooo", "I_ovov": "ovov", "I_voov": "voov", "I_vovv_p": "vovv", "I_ooov_p": "ooov", "r1": "ov",
    "r2": "oovv", "D1": "ov", "D2": "oovv", "t1": "ov", "t2": "oovv",
    # what a split update leaves (include/afesp.h); "p": the v (v + 1) / 2 column pairs a <= b of the packed ladder, p = a + b (b + 1) / 2
    "r1_sh": "ov", "ooov_sh": "ooov", "pp": "oop",
}


@dataclasses.dataclass
class FcidumpHeader:
    norb: int       # as the header says: spatial orbitals, or spin orbitals with uhf
    nelec: int
    ms2: int
    uhf: bool
    nlines: int     # non-blank lines after the header


@dataclasses.dataclass
class FcidumpIn:
    """What Engine.read_fcidump returns.  Closed shell: h / fock / levels; open shell: the _a / _b pairs.  Matrices are [n, n] over the
    n spatial orbitals of the file and symmetric to the bit; the eri_* arrays are there with want_eri=True."""
    norb: int
    nelec: int
    ms2: int
    uhf: bool
    e_core: float
    e_ref: float
    fock_offdiag: float
    nread: int
    h: np.ndarray | None = None
    fock: np.ndarray | None = None
    levels: np.ndarray | None = None
    h_a: np.ndarray | None = None
    h_b: np.ndarray | None = None
    fock_a: np.ndarray | None = None
    fock_b: np.ndarray | None = None
    levels_a: np.ndarray | None = None
    levels_b: np.ndarray | None = None
    eri: np.ndarray | None = None
    eri_aa: np.ndarray | None = None
    eri_ab: np.ndarray | None = None      # [npair, npair], row: alpha pair
    eri_bb: np.ndarray | None = None
    # a restricted open-shell file (Engine.read_fcidump_rohf): h, fock_a / fock_b, eri, and max |F| over both spins of the occupied-occupied
    # off-diagonal, the virtual-virtual off-diagonal and the occupied-virtual elements
    fock_offdiag3: tuple | None = None

    @property
    def nspatial(self) -> int:
        return self.norb // 2 if self.uhf else self.norb

    @property
    def nalpha(self) -> int:
        return (self.nelec + self.ms2) // 2

    @property
    def nbeta(self) -> int:
        return (self.nelec - self.ms2) // 2


def scan_fcidump(path) -> FcidumpHeader:
    """The header of a FCIDUMP and the number of lines after it (afesp_fcidump_scan: host only, no GPU context)."""
    norb, nelec, ms2, uhf, nl = i64(), i64(), i64(), C.c_int(), i64()
    rc = load_library().afesp_fcidump_scan(str(path).encode(), C.byref(norb), C.byref(nelec), C.byref(ms2), C.byref(uhf), C.byref(nl))
    if rc != 0:
        raise AfespError(f"status {rc}: afesp_fcidump_scan: {path} is unreadable or has no &FCI ... &END header with NORB and NELEC")
    return FcidumpHeader(norb.value, nelec.value, ms2.value, bool(uhf.value), nl.value)


def device_count():
    """Number of HIP devices this process sees (afesp_device_count; 0 without a GPU)."""
    return int(load_library().afesp_device_count())


def first_use_count():
    """Launch sites of this process that resolved their kernel under the first-use lock so far (afesp_first_use_count; test hook)."""
    return int(load_library().afesp_first_use_count())


class Engine:
    """One GPU context.  Method names follow the reference routines they replace."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.afesp_ctx_create(device, C.byref(h))
        if rc != 0:
            raise AfespError(f"afesp_ctx_create(device={device}) failed with status {rc} "
                             "(no usable MI355X/HIP device; the accelerated path has no CPU fallback)")
        self.h = h
        self.o = self.v = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.afesp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise AfespError(f"status {rc}: {self.L.afesp_last_error(self.h).decode()}")

    # ---- src/mp2.f90:261-449
    def do_mp2_spatial(self, nbasis, nocc, canon_coeff, canon_levels, eri_packed, want_eri_mo=True):
        e2 = dbl(0.0)
        out = np.zeros(self.L.afesp_neri(nbasis)) if want_eri_mo else None
        src = None   # None: the AO integrals read_eri_text left on the device
        if eri_packed is not None:
            eri_packed = np.ascontiguousarray(eri_packed, dtype=np.float64)
            src = eri_packed.ctypes.data_as(C.c_void_p)
        self._chk(self.L.afesp_ao2mo_mp2(self.h, nbasis, nocc, _f(canon_coeff), _f(canon_levels), src,
                                         out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(e2)))
        return e2.value, out

    # ---- src/ccsd.f90:279-402
    def ccsd_init(self, nocc, nvirt, canon_levels, eri_mo_packed=None, diis_n_errmat=8):
        self.o, self.v = int(nocc), int(nvirt)
        ptr = None
        if eri_mo_packed is not None:
            eri_mo_packed = np.ascontiguousarray(eri_mo_packed, dtype=np.float64)
            ptr = eri_mo_packed.ctypes.data_as(C.c_void_p)
        self._chk(self.L.afesp_ccsd_init(self.h, nocc, nvirt, ptr, _f(canon_levels), diis_n_errmat))

    def synthetic_init(self, nocc, nvirt, scale=0.02, seed=12345, diis_n_errmat=8):
        self.o, self.v = int(nocc), int(nvirt)
        self._chk(self.L.afesp_synthetic_init(self.h, nocc, nvirt, scale, seed, diis_n_errmat))

    def ccsd_energy(self, e_tol=1e-6, t_tol=1e-7):
        e, r, c = dbl(), dbl(), C.c_int()
        self._chk(self.L.afesp_ccsd_energy(self.h, e_tol, t_tol, C.byref(e), C.byref(r), C.byref(c)))
        return e.value, r.value, bool(c.value)

    def ccsd_iterate(self, e_tol=1e-6, t_tol=1e-7):
        e, r, c = dbl(), dbl(), C.c_int()
        self._chk(self.L.afesp_ccsd_iterate(self.h, e_tol, t_tol, C.byref(e), C.byref(r), C.byref(c)))
        return e.value, r.value, bool(c.value)

    def ccsd_diis(self):
        self._chk(self.L.afesp_ccsd_diis(self.h))

    def update_intermediates(self):
        self._chk(self.L.afesp_ccsd_update_intermediates(self.h))

    def update_amplitudes(self):
        self._chk(self.L.afesp_ccsd_update_amplitudes(self.h))

    def do_ccsd_spatial(self, maxiter=50, e_tol=1e-6, t_tol=1e-7):
        en = np.zeros(maxiter + 1)
        rm = np.zeros(maxiter + 1)
        nit = C.c_int()
        self._chk(self.L.afesp_ccsd_solve(self.h, maxiter, e_tol, t_tol, en, rm, C.byref(nit)))
        return nit.value, en, rm

    def amplitudes(self):
        o, v = self.o, self.v
        t1 = np.zeros(o * v)
        t2 = np.zeros(o * o * v * v)
        self._chk(self.L.afesp_ccsd_get_amplitudes(self.h, t1, t2))
        return t1.reshape((o, v), order="F"), t2.reshape((o, o, v, v), order="F")

    def set_amplitudes(self, t1, t2):
        self._chk(self.L.afesp_ccsd_set_amplitudes(self.h, _f(t1), _f(t2)))

    def tensor(self, name):
        ext = {"o": self.o, "v": self.v, "p": self.v * (self.v + 1) // 2}
        dims = tuple(ext[ch] for ch in TENSOR_SHAPES[name])
        buf = np.zeros(int(np.prod(dims)))
        self._chk(self.L.afesp_ccsd_get_tensor(self.h, name.encode(), buf, buf.size))
        return buf.reshape(dims, order="F")

    # ---- src/ccsd.f90:2018-2293
    def ntriples(self):
        return self.L.afesp_ccsd_t_ntriples(self.o)

    def shard_bounds(self, world, cr=False):
        """Cost-balanced shard boundaries of the (i<=j<=k) list: rank r evaluates [b[r], b[r+1])."""
        b = (i64 * (world + 1))()
        self._chk(self.L.afesp_ccsd_t_shard_bounds(self.h, self.o, self.v, 1 if cr else 0, world, b))
        return [int(x) for x in b]

    def do_ccsd_t_spatial(self, t_begin=0, t_end=None):
        out = np.zeros(4)
        if t_end is None:
            t_end = self.ntriples()
        self._chk(self.L.afesp_ccsd_t(self.h, t_begin, t_end, out))
        return out

    # ---- multi-GPU: the OpenMP reduction of src/ccsd.f90:2091 as a sum over ranks (include/afesp.h)
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        rc = self.L.afesp_comm_unique_id(buf)
        if rc != 0:
            raise AfespError(f"afesp_comm_unique_id failed with status {rc} (is librccl.so.1 loadable?)")
        return buf.raw

    def comm_init(self, rank, world, transport=COMM_RCCL, bootstrap_path=None, unique_id=None):
        self._chk(self.L.afesp_comm_init(self.h, rank, world, transport,
                                         None if bootstrap_path is None else str(bootstrap_path).encode(), unique_id))

    def comm_destroy(self):
        self._chk(self.L.afesp_comm_destroy(self.h))

    def allreduce_sum(self, values):
        buf = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._chk(self.L.afesp_allreduce_sum(self.h, buf, buf.size))
        return buf

    def t_block_size(self, cr=False):
        sb = C.c_int()
        self._chk(self.L.afesp_ccsd_t_block_size(self.h, self.o, self.v, 1 if cr else 0, C.byref(sb)))
        return sb.value

    def arena_stats(self):
        out = np.zeros(4)
        self._chk(self.L.afesp_arena_stats(self.h, out))
        return dict(driver_calls=int(out[0]), reuse_hits=int(out[1]), idle_gb=out[2] / 1e9, live_gb=out[3] / 1e9)

    def launch_counts(self):
        """launches so far in this context: tall (streamed tall x skinny kernel), gett (gather kernel through the planner), tgemm
        (LDS-DMA GEMM, 128-row tiles), tgemm_mixed (... with 96-row tiles where the rows end)"""
        out = (C.c_uint64 * 4)()
        self._chk(self.L.afesp_launch_counts(self.h, out))
        return dict(tall=int(out[0]), gett=int(out[1]), tgemm=int(out[2]), tgemm_mixed=int(out[3]))

    def ccsd_set_split(self, mode):
        """1: split the CCSD iteration over the ranks, 0: replicas, -1: as AFESP_CC_SHARD says (default replicas)."""
        self._chk(self.L.afesp_ccsd_set_split(self.h, int(mode)))

    def ccsd_set_fused(self, mode):
        """1: the launch-fused iteration of small systems (csrc/fused.h), 0: call by call, -1: as AFESP_FUSED says (default on)."""
        self._chk(self.L.afesp_ccsd_set_fused(self.h, int(mode)))

    def ccsd_iteration_launches(self):
        """Kernel launches of one compiled (launch-fused) iteration; 0 when the iteration runs call by call."""
        n = C.c_int()
        self._chk(self.L.afesp_ccsd_iteration_launches(self.h, C.byref(n)))
        return n.value

    def ccsd_is_split(self):
        f = C.c_int()
        self._chk(self.L.afesp_ccsd_is_split(self.h, C.byref(f)))
        return bool(f.value)

    def test_inject(self, what):
        self._chk(self.L.afesp_test_inject(self.h, what))

    # ---- test hook: the block Davidson unit on A = diag(d) + U V^T given as data (include/afesp.h; tests/test_gpu_davidson.py).
    # Vectors are whole (nvec,) arrays here; the metric's split at n1 is made in these wrappers.
    davidson_test_shape = (0, 1, 1, 2)                                     # (n1, nvec, nroots, max_space) of the last create
    davidson_test_complex = False                                          # the last start was davidson_test_linear_start_complex

    def davidson_test_create(self, n1, nvec, w2, follow, nroots, max_space, d, U, V, diag):
        """U, V: (nvec, r) or None (r = 0)"""
        r = 0 if U is None else np.asarray(U).shape[1]
        Uf, Vf = (_f(U), _f(V)) if r else (np.zeros(1), np.zeros(1))
        self._chk(self.L.afesp_test_davidson_create(self.h, n1, nvec, w2, 1 if follow else 0, nroots, max_space, r, _f(d), Uf, Vf, _f(diag)))
        self.davidson_test_shape = (int(n1), int(nvec), int(nroots), int(max_space))
        self.davidson_test_complex = False

    def davidson_test_destroy(self):
        self._chk(self.L.afesp_test_davidson_destroy(self.h))   # (the shape stays: a later call gets the library's own refusal)

    def _davidson_halves(self, x):
        n1, nvec = self.davidson_test_shape[:2]
        x = _f(x)
        if x.size != nvec:
            raise ValueError("davidson_test: a vector has nvec elements")
        return (x[:n1].copy() if n1 else np.zeros(1)), (x[n1:].copy() if n1 < nvec else np.zeros(1))

    def davidson_test_set_guess(self, k, x):
        self._chk(self.L.afesp_test_davidson_set_guess(self.h, k, *self._davidson_halves(x)))
        self.davidson_test_complex = False

    def davidson_test_iterate(self, tol=1e-8):
        """One step -> (omega, resnorm, flags, dict(nsigma, ncollapse, nb, npend), converged)"""
        nroots = self.davidson_test_shape[2]
        om, rs = np.zeros(nroots), np.zeros(nroots)
        fl, cnt, cv = (C.c_int * nroots)(), (C.c_int * 4)(), C.c_int()
        self._chk(self.L.afesp_test_davidson_iterate(self.h, tol, om, rs, fl, cnt, C.byref(cv)))
        return om, rs, np.array(fl[:], dtype=int), dict(zip(("nsigma", "ncollapse", "nb", "npend"), cnt[:])), bool(cv.value)

    def davidson_test_linear_start(self, rhs, shifts):
        """rhs: (nvec, nrhs); shifts: nroots of them"""
        rhs = np.asarray(rhs, dtype=np.float64)
        self._chk(self.L.afesp_test_davidson_linear_start(self.h, rhs.shape[1], _f(rhs), _f(shifts)))
        self.davidson_test_complex = False

    def davidson_test_linear_start_complex(self, rhs, shifts):
        """rhs: (nvec, nrhs); shifts: nroots complex numbers.  davidson_test_linear_iterate then makes the complex steps, and
        davidson_test_fetch gives x, sx, corr as complex (nvec, nroots) arrays and y as (complex coefficients (nb, nroots), shifts)"""
        rhs = np.asarray(rhs, dtype=np.float64)
        z = np.asarray(shifts, dtype=np.complex128)
        self._chk(self.L.afesp_test_davidson_linear_start_complex(self.h, rhs.shape[1], _f(rhs), np.ascontiguousarray(z.real),
                                                                  np.ascontiguousarray(z.imag)))
        self.davidson_test_complex = True

    def davidson_test_linear_iterate(self, tol=1e-8):
        """One step -> (resnorm, flags, dict(nsigma, ncollapse, nb, npend), converged)"""
        nroots = self.davidson_test_shape[2]
        rs = np.zeros(nroots)
        fl, cnt, cv = (C.c_int * nroots)(), (C.c_int * 4)(), C.c_int()
        self._chk(self.L.afesp_test_davidson_linear_iterate(self.h, tol, rs, fl, cnt, C.byref(cv)))
        return rs, np.array(fl[:], dtype=int), dict(zip(("nsigma", "ncollapse", "nb", "npend"), cnt[:])), bool(cv.value)

    def davidson_test_get_vector(self, k):
        n1, nvec = self.davidson_test_shape[:2]
        x1, x2 = np.zeros(max(n1, 1)), np.zeros(max(nvec - n1, 1))
        self._chk(self.L.afesp_test_davidson_get_vector(self.h, k, x1, x2))
        return np.concatenate([x1[:n1], x2[:nvec - n1]])

    def davidson_test_fetch(self, what):
        """What the state holds (include/afesp.h): vectors as the columns of an (nvec, k) array, G (nb, nb), prhs (nb, nrhs), y ->
        (coefficients (nb, nr), omega (nr,)), counts -> dict, diag / target flat"""
        n1, nvec, nroots, ms = self.davidson_test_shape
        cz = self.davidson_test_complex
        ncol = 2 if cz else 1
        cap = {"G": ms * ms, "prhs": ms * nroots, "y": (ms + 1) * nroots * ncol, "target": nroots, "counts": 4, "diag": nvec,
               "B": nvec * ms, "S": nvec * ms}.get(what, nvec * nroots * ncol)
        if what in ("B", "S", "pend"):
            c = self.davidson_test_fetch("counts")
            cap = nvec * (c["npend"] if what == "pend" else c["nb"])
        out, n = np.zeros(max(cap, 1)), i64()
        self._chk(self.L.afesp_test_davidson_fetch(self.h, what.encode(), out, cap, C.byref(n)))
        out = out[:n.value]
        if what == "counts":
            return dict(zip(("nsigma", "ncollapse", "nb", "npend"), (int(v) for v in out)))
        if cz and what in ("x", "sx", "corr"):
            cols = out.reshape(nvec, -1, order="F")
            return cols[:, 0::2] + 1j * cols[:, 1::2]
        if what in ("B", "S", "pend", "x", "sx", "corr"):
            return out.reshape(nvec, -1, order="F")
        if what == "G":
            nb = int(round(np.sqrt(out.size)))
            return out.reshape(nb, nb, order="F")
        if what == "prhs":
            nb = self.davidson_test_fetch("counts")["nb"]
            return out.reshape(nb, -1, order="F") if nb else out.reshape(0, 0)
        if what == "y":
            nb = self.davidson_test_fetch("counts")["nb"]
            if cz:
                nr = out.size // (2 * (nb + 1))
                y = out[:nb * nr].reshape(nb, nr, order="F") + 1j * out[nb * nr:2 * nb * nr].reshape(nb, nr, order="F")
                return y, out[2 * nb * nr:2 * nb * nr + nr] + 1j * out[2 * nb * nr + nr:]
            nr = out.size // (nb + 1)
            return out[:nb * nr].reshape(nb, nr, order="F"), out[nb * nr:]
        return out

    # ---- input / output side: src/integrals.f90:146-161, src/mp2.f90:451-487
    def read_eri_text(self, path, nbasis, want_host_copy=True):
        """-> (packed AO integrals or None, number of lines); the packed array also stays on the device."""
        out = np.zeros(self.L.afesp_neri(nbasis)) if want_host_copy else None
        n = i64()
        self._chk(self.L.afesp_read_eri_text(self.h, str(path).encode(), nbasis,
                                             out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(n)))
        return out, n.value

    def set_eri(self, nbasis, eri_packed):
        self._chk(self.L.afesp_set_eri(self.h, nbasis, np.ascontiguousarray(eri_packed, dtype=np.float64)))

    def build_fock(self, nbasis, density, core_hamil):
        """src/hf.f90:349-385 on the device-resident packed AO integrals."""
        out = np.zeros(nbasis * nbasis)
        self._chk(self.L.afesp_build_fock(self.h, nbasis, _f(density), _f(core_hamil), out))
        return out.reshape((nbasis, nbasis), order="F")

    def build_fock_uhf(self, nbasis, dens_a, dens_b, core_hamil):
        """F_s = H + J[Da + Db] - K[D_s] (s = alpha, beta) on the device-resident packed AO integrals -> (F_alpha, F_beta)."""
        fa, fb = np.zeros(nbasis * nbasis), np.zeros(nbasis * nbasis)
        self._chk(self.L.afesp_build_fock_uhf(self.h, nbasis, _f(dens_a), _f(dens_b), _f(core_hamil), fa, fb))
        return fa.reshape((nbasis, nbasis), order="F"), fb.reshape((nbasis, nbasis), order="F")

    def do_ump2(self, nbasis, nalpha, nbeta, coeff_a, coeff_b, levels_a, levels_b, eri_packed=None, want_eri_mo=True):
        """-> (E(UMP2), (aa|aa) packed, (aa|bb) as [npair, npair] (row: alpha pair), (bb|bb) packed); the three blocks stay on
        the device for init_cc_uspinorb.  eri_packed None: the AO integrals set_eri / read_eri_text left there."""
        e2 = dbl(0.0)
        npr = nbasis * (nbasis + 1) // 2
        aa = np.zeros(self.L.afesp_neri(nbasis)) if want_eri_mo else None
        bb = np.zeros(self.L.afesp_neri(nbasis)) if want_eri_mo else None
        ab = np.zeros(npr * npr) if want_eri_mo else None
        src = None
        if eri_packed is not None:
            eri_packed = np.ascontiguousarray(eri_packed, dtype=np.float64)
            src = eri_packed.ctypes.data_as(C.c_void_p)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.L.afesp_ao2mo_ump2(self.h, nbasis, nalpha, nbeta, _f(coeff_a), _f(coeff_b),
                                          np.ascontiguousarray(levels_a, dtype=np.float64), np.ascontiguousarray(levels_b, dtype=np.float64),
                                          src, ptr(aa), ptr(ab), ptr(bb), C.byref(e2)))
        return e2.value, aa, (ab.reshape((npr, npr)) if ab is not None else None), bb

    def init_cc_uspinorb(self, nbasis, nalpha, nbeta, levels_a, levels_b, diis_nerr=8):
        """The spin-orbital state from the blocks do_ump2 left; then the so_* methods drive it (occupied: alpha then beta,
        virtual: alpha then beta)."""
        self.so_o = int(nalpha + nbeta)
        self.so_v = int(2 * nbasis - self.so_o)
        self._chk(self.L.afesp_ccsd_uso_init(self.h, nbasis, nalpha, nbeta, np.ascontiguousarray(levels_a, dtype=np.float64),
                                             np.ascontiguousarray(levels_b, dtype=np.float64), diis_nerr))

    # ---- frozen core / frozen virtuals: the active orbital window [nfc, nbasis - nfv)
    def mo_window(self, nbasis, nocc, nfc, nfv, canon_levels, eri_mo=None, want_eri=True):
        """-> (packed MO integrals over the n_act = nbasis - nfc - nfv active orbitals or None, frozen-core E(MP2)).  eri_mo None: the
        integrals do_mp2_spatial left on the device.  The window stays resident as do_mp2_spatial leaves a basis of n_act functions:
        ccsd_init(nocc - nfc, nvirt - nfv, canon_levels[nfc:nbasis - nfv]) / init_cc_spinorb(n_act, nel - 2 nfc, ...) follow."""
        e2 = dbl(0.0)
        n_act = int(nbasis) - int(nfc) - int(nfv)
        out = np.zeros(self.L.afesp_neri(n_act)) if want_eri and 0 < n_act <= nbasis else None
        src = None
        if eri_mo is not None:
            eri_mo = np.ascontiguousarray(eri_mo, dtype=np.float64)
            src = eri_mo.ctypes.data_as(C.c_void_p)
        self._chk(self.L.afesp_mo_window(self.h, nbasis, nocc, nfc, nfv, np.ascontiguousarray(canon_levels, dtype=np.float64), src,
                                         out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(e2)))
        return out, e2.value

    def umo_window(self, nbasis, nalpha, nbeta, nfc, nfv, levels_a, levels_b, want_eri=True):
        """The same for the three blocks do_ump2 left -> ((aa|aa) packed, (aa|bb) as [npair_act, npair_act], (bb|bb) packed -- or
        Nones --, frozen-core E(UMP2)); init_cc_uspinorb(n_act, nalpha - nfc, nbeta - nfc, levels_a[nfc:], levels_b[nfc:]) follows."""
        e2 = dbl(0.0)
        n_act = int(nbasis) - int(nfc) - int(nfv)
        ok = want_eri and 0 < n_act <= nbasis
        npr = n_act * (n_act + 1) // 2
        aa = np.zeros(self.L.afesp_neri(n_act)) if ok else None
        bb = np.zeros(self.L.afesp_neri(n_act)) if ok else None
        ab = np.zeros(npr * npr) if ok else None
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.L.afesp_umo_window(self.h, nbasis, nalpha, nbeta, nfc, nfv, np.ascontiguousarray(levels_a, dtype=np.float64),
                                          np.ascontiguousarray(levels_b, dtype=np.float64), ptr(aa), ptr(ab), ptr(bb), C.byref(e2)))
        return aa, (ab.reshape((npr, npr)) if ab is not None else None), bb, e2.value

    # ---- frozen natural orbitals (afesp_amd/fno.py does the host algebra)
    def mp2_vv_density(self, nbasis, nocc, nfc, canon_levels):
        """-> (D[v, v], frozen-core E(MP2) of the full virtual space) from the MO integrals do_mp2_spatial left on the device, before any
        window: D(a,b) = sum_ijc [2 t(ijac) - t(ijca)] t(ijbc) over the active occupied orbitals, symmetric to the bit."""
        e2 = dbl(0.0)
        v = max(int(nbasis) - int(nocc), 0)
        d = np.zeros(v * v)
        self._chk(self.L.afesp_mp2_vv_density(self.h, nbasis, nocc, nfc, np.ascontiguousarray(canon_levels, dtype=np.float64), d,
                                              C.byref(e2)))
        return d.reshape((v, v), order="F"), e2.value

    def ump2_vv_density(self, nbasis, nalpha, nbeta, nfc, levels_a, levels_b):
        """-> (D_alpha[va, va], D_beta[vb, vb], frozen-core E(UMP2)) from the three blocks do_ump2 left on the device."""
        e2 = dbl(0.0)
        va, vb = max(int(nbasis) - int(nalpha), 0), max(int(nbasis) - int(nbeta), 0)
        da, db = np.zeros(va * va), np.zeros(vb * vb)
        self._chk(self.L.afesp_ump2_vv_density(self.h, nbasis, nalpha, nbeta, nfc, np.ascontiguousarray(levels_a, dtype=np.float64),
                                               np.ascontiguousarray(levels_b, dtype=np.float64), da, db, C.byref(e2)))
        return da.reshape((va, va), order="F"), db.reshape((vb, vb), order="F"), e2.value

    def fno_window(self, nbasis, nocc, nfc, canon_coeff, canon_levels, eri_packed=None, n_keep=None, occ_tol=0.0, report=print):
        """The whole frozen-natural-orbital set-up of a closed shell: transform with the canonical orbitals, the MP2 virtual density, the
        natural virtuals (fno.natural_virtuals), a second transform with the rotated coefficients on the AO integrals resident on the
        device, and the window (nfc, v - n_keep).  -> (n_keep, occupations, levels_act, E(MP2) in the FNO space, Delta MP2); afterwards
        ccsd_init(nocc - nfc, n_keep, levels_act) / init_cc_spinorb(nocc - nfc + n_keep, 2 (nocc - nfc), levels_act).  The rotated
        orbitals stay in self.fno_coeff / self.fno_levels.  eri_packed None: the AO integrals set_eri / read_eri_text left there."""
        from . import fno
        if eri_packed is not None:
            self.set_eri(nbasis, eri_packed)
        self.do_mp2_spatial(nbasis, nocc, canon_coeff, canon_levels, None, want_eri_mo=False)
        d, e_full = self.mp2_vv_density(nbasis, nocc, nfc, canon_levels)
        kept, occ, c2, l2 = fno.natural_virtuals(d, canon_coeff, canon_levels, nocc, n_keep, occ_tol, report)
        self.fno_coeff, self.fno_levels = c2, l2
        nfv = nbasis - nocc - kept
        self.do_mp2_spatial(nbasis, nocc, c2, l2, None, want_eri_mo=False)   # (its own E(MP2) is not meaningful: Fock is not diagonal)
        _, e_fno = self.mo_window(nbasis, nocc, nfc, nfv, l2, want_eri=False)
        return kept, occ, np.ascontiguousarray(l2[nfc:nbasis - nfv]), e_fno, e_full - e_fno

    def ufno_window(self, nbasis, nalpha, nbeta, nfc, coeff_a, coeff_b, levels_a, levels_b, eri_packed=None, n_keep=None, occ_tol=0.0,
                    report=print):
        """The open-shell twin -> (n_keep, (occ_a, occ_b), (levels_act_a, levels_act_b), E(UMP2) in the FNO space, Delta MP2); n_keep
        counts the natural virtuals kept in the smaller virtual space, the same number min(va, vb) - n_keep is dropped from both spins.
        Afterwards init_cc_uspinorb(nbasis - nfc - n_drop, nalpha - nfc, nbeta - nfc, *levels_act)."""
        from . import fno
        if eri_packed is not None:
            self.set_eri(nbasis, eri_packed)
        self.do_ump2(nbasis, nalpha, nbeta, coeff_a, coeff_b, levels_a, levels_b, None, want_eri_mo=False)
        da, db, e_full = self.ump2_vv_density(nbasis, nalpha, nbeta, nfc, levels_a, levels_b)
        kept, occ, ca, cb, la, lb = fno.natural_virtuals_uhf(da, db, coeff_a, coeff_b, levels_a, levels_b, nalpha, nbeta, n_keep, occ_tol,
                                                             report)
        self.fno_coeff, self.fno_levels = (ca, cb), (la, lb)
        nfv = nbasis - max(nalpha, nbeta) - kept
        self.do_ump2(nbasis, nalpha, nbeta, ca, cb, la, lb, None, want_eri_mo=False)
        *_, e_fno = self.umo_window(nbasis, nalpha, nbeta, nfc, nfv, la, lb, want_eri=False)
        hi = nbasis - nfv
        return kept, occ, (np.ascontiguousarray(la[nfc:hi]), np.ascontiguousarray(lb[nfc:hi])), e_fno, e_full - e_fno

    def write_fcidump(self, path, nbasis):
        n = i64()
        self._chk(self.L.afesp_write_fcidump(self.h, str(path).encode(), nbasis, C.byref(n)))
        return n.value

    # ---- the active space as a standard FCIDUMP (afesp_amd/fcidump.py reads it back)
    def core_operator(self, nbasis, nfc, nfv, canon_coeff, core_hamil):
        """-> (h_act[n_act, n_act], e_core) of the window [nfc, nbasis - nfv) from the full MO integrals do_mp2_spatial left on the
        device, BEFORE mo_window: h_act = h_mo + sum_c [2 (pq|cc) - (pc|qc)], e_core = 2 sum_c h_cc + sum_cd [2 (cc|dd) - (cd|cd)]
        (electronic; the caller adds the nuclear repulsion).  h_act is symmetric to the bit."""
        e = dbl(0.0)
        na = max(int(nbasis) - int(nfc) - int(nfv), 0)
        h = np.zeros(na * na)
        self._chk(self.L.afesp_core_operator(self.h, nbasis, nfc, nfv, _f(canon_coeff), _f(core_hamil), h, C.byref(e)))
        return h.reshape((na, na), order="F"), e.value

    def ucore_operator(self, nbasis, nfc, nfv, coeff_a, coeff_b, core_hamil):
        """The open-shell twin on the three blocks do_ump2 left, before umo_window -> (h_act_alpha, h_act_beta, e_core)."""
        e = dbl(0.0)
        na = max(int(nbasis) - int(nfc) - int(nfv), 0)
        ha, hb = np.zeros(na * na), np.zeros(na * na)
        self._chk(self.L.afesp_ucore_operator(self.h, nbasis, nfc, nfv, _f(coeff_a), _f(coeff_b), _f(core_hamil), ha, hb, C.byref(e)))
        return ha.reshape((na, na), order="F"), hb.reshape((na, na), order="F"), e.value

    def write_fcidump_active(self, path, n_act, nelec_act, ms2, h_act, e_core_total, threshold=1e-12):
        """The integrals resident for n_act orbitals (the window after mo_window, else the full basis), h_act and e_core_total (core
        energy plus nuclear repulsion) as a standard FCIDUMP -> number of lines after the header."""
        n = i64()
        self._chk(self.L.afesp_write_fcidump_active(self.h, str(path).encode(), n_act, nelec_act, ms2, _f(h_act), e_core_total, threshold,
                                                    C.byref(n)))
        return n.value

    def write_fcidump_uactive(self, path, n_act, nalpha_act, nbeta_act, h_act_a, h_act_b, e_core_total, threshold=1e-12):
        """The same for the three blocks resident after do_ump2 / umo_window: UHF=.TRUE., 2 n_act interleaved spin orbitals."""
        n = i64()
        self._chk(self.L.afesp_write_fcidump_uactive(self.h, str(path).encode(), n_act, nalpha_act, nbeta_act, _f(h_act_a), _f(h_act_b),
                                                     e_core_total, threshold, C.byref(n)))
        return n.value

    # ---- a standard FCIDUMP as input
    def read_fcidump(self, path, canonical_tol=1e-6, want_eri=False) -> FcidumpIn:
        """Reads a FCIDUMP onto the device (afesp_read_fcidump, or afesp_read_fcidump_uhf where the header says UHF=.TRUE.): the integrals
        are then resident as do_mp2_spatial / do_ump2 leave theirs, the orbitals in file order with the first nelec / 2 (nalpha, nbeta)
        occupied.  Raises AfespError where max |F(p,q)|, p != q, exceeds canonical_tol (the solvers assume canonical orbitals);
        canonical_tol=None skips that check."""
        hd = scan_fcidump(path)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ec, er, fo, nr = dbl(0.0), dbl(0.0), dbl(0.0), i64()
        if not hd.uhf:
            if hd.nelec % 2 or hd.ms2 != 0:
                raise AfespError("status 1: read_fcidump: an open shell without UHF=.TRUE. (restricted open-shell orbitals are not supported)")
            n, o = hd.norb, hd.nelec // 2
            h, f, lev = np.zeros(n * n), np.zeros(n * n), np.zeros(n)
            eri = np.zeros(self.L.afesp_neri(n)) if want_eri else None
            self._chk(self.L.afesp_read_fcidump(self.h, str(path).encode(), n, o, vp(h), vp(f), vp(lev), C.byref(ec), C.byref(er), C.byref(fo),
                                                vp(eri) if want_eri else None, C.byref(nr)))
            out = FcidumpIn(hd.norb, hd.nelec, hd.ms2, False, ec.value, er.value, fo.value, nr.value, h=h.reshape((n, n), order="F"),
                            fock=f.reshape((n, n), order="F"), levels=lev, eri=eri)
        else:
            if hd.norb % 2 or (hd.nelec + hd.ms2) % 2:
                raise AfespError("status 1: read_fcidump: UHF=.TRUE. with an odd NORB, or NELEC and MS2 of different parity")
            n, na, nb = hd.norb // 2, (hd.nelec + hd.ms2) // 2, (hd.nelec - hd.ms2) // 2
            m = [np.zeros(n * n) for _ in range(4)]
            la, lb = np.zeros(n), np.zeros(n)
            ne, npair = self.L.afesp_neri(n), n * (n + 1) // 2
            aa, bb, ab = (np.zeros(ne), np.zeros(ne), np.zeros(npair * npair)) if want_eri else (None, None, None)
            e = lambda a: vp(a) if want_eri else None
            self._chk(self.L.afesp_read_fcidump_uhf(self.h, str(path).encode(), n, na, nb, vp(m[0]), vp(m[1]), vp(m[2]), vp(m[3]), vp(la), vp(lb),
                                                    C.byref(ec), C.byref(er), C.byref(fo), e(aa), e(ab), e(bb), C.byref(nr)))
            sq = lambda a: a.reshape((n, n), order="F")
            out = FcidumpIn(hd.norb, hd.nelec, hd.ms2, True, ec.value, er.value, fo.value, nr.value, h_a=sq(m[0]), h_b=sq(m[1]), fock_a=sq(m[2]),
                            fock_b=sq(m[3]), levels_a=la, levels_b=lb, eri_aa=aa, eri_bb=bb,
                            eri_ab=ab.reshape((npair, npair)) if want_eri else None)
        if canonical_tol is not None and not out.fock_offdiag <= canonical_tol:
            raise AfespError(f"status 1: read_fcidump: the orbitals of {path} are not canonical: max |F(p,q)|, p != q, is "
                             f"{out.fock_offdiag:.3e}, above {canonical_tol:.1e} (the integrals are resident all the same)")
        return out

    # ---- restricted open-shell references (afesp_amd/rohf.py strings these together)
    def mo_fock_ro(self, nbasis, nalpha, nbeta, h_mo):
        """-> (F_alpha[n, n], F_beta[n, n], electronic reference energy) of the restricted determinant that fills the first nalpha / nbeta
        orbitals of the packed MO array resident for nbasis (do_mp2_spatial, read_fcidump, read_fcidump_rohf); symmetric to the bit."""
        n = int(nbasis)
        fa, fb, e = np.zeros(n * n), np.zeros(n * n), dbl(0.0)
        self._chk(self.L.afesp_mo_fock_ro(self.h, n, nalpha, nbeta, _f(h_mo), fa, fb, C.byref(e)))
        return fa.reshape((n, n), order="F"), fb.reshape((n, n), order="F"), e.value

    def read_fcidump_rohf(self, path, want_eri=False) -> FcidumpIn:
        """Reads a restricted FCIDUMP with MS2 >= 0 (no UHF flag) onto the device (afesp_read_fcidump_rohf): the packed array is resident as
        read_fcidump leaves it; fock_a / fock_b are the two spin Fock operators of the determinant, fock_offdiag3 their largest
        off-diagonal elements by block (reported, not judged: the orbitals of such a file are not canonical)."""
        hd = scan_fcidump(path)
        if hd.uhf or hd.ms2 < 0 or (hd.nelec + hd.ms2) % 2:
            raise AfespError("status 1: read_fcidump_rohf: needs a restricted file (no UHF=.TRUE.) with MS2 >= 0 of the parity of NELEC")
        n, na, nb = hd.norb, (hd.nelec + hd.ms2) // 2, (hd.nelec - hd.ms2) // 2
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ec, er, nr = dbl(0.0), dbl(0.0), i64()
        h, fa, fb, fo = np.zeros(n * n), np.zeros(n * n), np.zeros(n * n), np.zeros(3)
        eri = np.zeros(self.L.afesp_neri(n)) if want_eri else None
        self._chk(self.L.afesp_read_fcidump_rohf(self.h, str(path).encode(), n, na, nb, vp(h), vp(fa), vp(fb), C.byref(ec), C.byref(er), vp(fo),
                                                 vp(eri) if want_eri else None, C.byref(nr)))
        sq = lambda a: a.reshape((n, n), order="F")
        return FcidumpIn(hd.norb, hd.nelec, hd.ms2, False, ec.value, er.value, float(fo.max()), nr.value, h=sq(h), fock_a=sq(fa), fock_b=sq(fb),
                         eri=eri, fock_offdiag3=tuple(float(x) for x in fo))

    def mo_rotate_uhf(self, nbasis, u_a, u_b, want_eri=False):
        """The resident packed MO integrals rotated with u_a / u_b[new orbital, old orbital] into the three blocks do_ump2 leaves ->
        ((aa|aa) packed, (aa|bb) as [npair, npair], (bb|bb) packed) or Nones; init_cc_uspinorb / uso_init_fock / umo_window follow."""
        n = int(nbasis)
        npr = n * (n + 1) // 2
        aa = np.zeros(self.L.afesp_neri(n)) if want_eri else None
        bb = np.zeros(self.L.afesp_neri(n)) if want_eri else None
        ab = np.zeros(npr * npr) if want_eri else None
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        self._chk(self.L.afesp_mo_rotate_uhf(self.h, n, _f(u_a), _f(u_b), ptr(aa), ptr(ab), ptr(bb)))
        return aa, (ab.reshape((npr, npr)) if ab is not None else None), bb

    def uso_init_fock(self, nbasis, nalpha, nbeta, fock_a, fock_b, diis_nerr=8):
        """The spin-orbital state of init_cc_uspinorb from the resident three blocks with the full spin Fock matrices of the same orbitals
        (levels: their diagonals; f_ov and the off-diagonal f_oo / f_vv enter the equations) -> sum f_ia^2 / D_ia + 1/4 sum <ij||ab>^2 /
        D_ijab, in semicanonical orbitals the ROHF-MBPT(2) energy.  The so_* methods drive the state."""
        self.so_o = int(nalpha + nbeta)
        self.so_v = int(2 * nbasis - self.so_o)
        e2 = dbl(0.0)
        self._chk(self.L.afesp_ccsd_uso_init_fock(self.h, nbasis, nalpha, nbeta, _f(fock_a), _f(fock_b), diis_nerr, C.byref(e2)))
        return e2.value

    # ---- spin-orbital path: do_ccsd_spinorb (src/ccsd.f90:71-277), do_ccsd_t_spinorb (:1812-1922)
    SO_SHAPES = {"F_vv": "vv", "F_oo": "oo", "F_ov": "ov", "W_oooo": "oooo", "W_vvvv": "vvvv", "W_ovvo": "ovvo", "tau": "oovv",
                 "tau_tilde": "oovv", "oovv": "oovv", "vvvv": "vvvv", "t1": "ov", "t2": "oovv", "f_ov": "ov", "f_oo": "oo", "f_vv": "vv",
                 "D1": "ov",      # the singles denominators e_i - e_a
                 # of a live Lambda state (status 21 otherwise): H_vvvo is H_abei stored (i,e,a,b), H_ovoo is H_mbij stored (m,b,i,j)
                 "H_ov": "ov", "H_oo": "oo", "H_vv": "vv", "H_oooo": "oooo", "H_vovv": "vovv", "H_ooov": "ooov", "H_ovvo": "ovvo",
                 "H_vvvo": "ovvv", "H_ovoo": "ovoo", "lam_tau": "oovv", "G_vv": "vv", "G_oo": "oo"}

    def init_cc_spinorb(self, nbasis, nel, canon_levels, eri_mo=None, diis_nerr=8, foo_as_published=False):
        self.so_o, self.so_v = int(nel), int(2 * nbasis - nel)
        eri = None
        if eri_mo is not None:
            eri_mo = np.ascontiguousarray(eri_mo, dtype=np.float64)
            eri = eri_mo.ctypes.data_as(C.c_void_p)
        self._chk(self.L.afesp_ccsd_so_init(self.h, nbasis, nel, eri, np.ascontiguousarray(canon_levels, dtype=np.float64),
                                            diis_nerr, 1 if foo_as_published else 0))

    def _so_step(self, fn, e_tol, t_tol):
        e, r, c = dbl(), dbl(), C.c_int()
        self._chk(fn(self.h, e_tol, t_tol, C.byref(e), C.byref(r), C.byref(c)))
        return e.value, r.value, bool(c.value)

    def so_energy(self, e_tol=1e-6, t_tol=1e-7):
        return self._so_step(self.L.afesp_ccsd_so_energy, e_tol, t_tol)

    def so_iterate(self, e_tol=1e-6, t_tol=1e-7):
        return self._so_step(self.L.afesp_ccsd_so_iterate, e_tol, t_tol)

    def so_diis(self):
        self._chk(self.L.afesp_ccsd_so_diis(self.h))

    def do_ccsd_spinorb(self, maxiter=50, e_tol=1e-6, t_tol=1e-7):
        """The driver loop of src/ccsd.f90:215-275 -> (iterations or -1, energies incl. the MP1 line, un-rooted rms)."""
        en, rm = [], []
        e, r, _ = self.so_energy(e_tol, t_tol)
        en.append(e); rm.append(r)
        for it in range(1, maxiter + 1):
            e, r, conv = self.so_iterate(e_tol, t_tol)
            en.append(e); rm.append(r)
            if conv:
                return it, np.array(en), np.array(rm)
            self.so_diis()
        return -1, np.array(en), np.array(rm)

    def so_amplitudes(self):
        o, v = self.so_o, self.so_v
        t1 = np.zeros(o * v)
        t2 = np.zeros(o * o * v * v)
        self._chk(self.L.afesp_ccsd_so_get_amplitudes(self.h, t1, t2))
        return t1.reshape((o, v), order="F"), t2.reshape((o, o, v, v), order="F")

    def so_set_amplitudes(self, t1, t2):
        self._chk(self.L.afesp_ccsd_so_set_amplitudes(self.h, _f(t1), _f(t2)))

    def so_tensor(self, name):
        dims = tuple(self.so_o if ch == "o" else self.so_v for ch in self.SO_SHAPES[name])
        buf = np.zeros(int(np.prod(dims)))
        self._chk(self.L.afesp_ccsd_so_get_tensor(self.h, name.encode(), buf, buf.size))
        return buf.reshape(dims, order="F")

    def so_levels(self):
        """The levels of the state's o + v spin orbitals relative to the first virtual one (from the singles denominators e_i - e_a):
        every difference of levels is that of the state"""
        d1 = self.so_tensor("D1")
        return np.concatenate([d1[:, 0], d1[0, 0] - d1[0, :]])

    def so_abs_levels(self):
        """The levels of the state's o + v spin orbitals themselves, occupied first (so_levels gives them relative to the first virtual one,
        which serves differences of as many occupied as virtual levels only)"""
        buf = np.zeros(self.so_o + self.so_v)
        self._chk(self.L.afesp_ccsd_so_get_tensor(self.h, b"levels", buf, buf.size))
        return buf

    def so_ntriples(self):
        return self.L.afesp_ccsd_so_t_ntriples(self.so_o)

    def do_ccsd_t_spinorb(self, t_begin=0, t_end=None):
        if t_end is None:
            t_end = self.so_ntriples()
        e = dbl()
        self._chk(self.L.afesp_ccsd_so_t(self.h, t_begin, t_end, C.byref(e)))
        return e.value

    # ---- Lambda and the unrelaxed one-particle density of the spin-orbital state (include/afesp.h; afesp_amd.density drives them)
    def so_lambda_init(self, diis_nerr=8):
        """The t-dependent intermediates from the state's current t1 / t2 and l = t.  Whatever changes t1 / t2 afterwards makes the Lambda
        state stale (status 21)."""
        self._chk(self.L.afesp_ccsd_so_lambda_init(self.h, diis_nerr))

    def so_lambda_iterate(self, e_tol=1e-6, l_tol=1e-7):
        """One Jacobi step -> (pseudo energy, sum (l2 - l2_old)^2, converged)"""
        return self._so_step(self.L.afesp_ccsd_so_lambda_iterate, e_tol, l_tol)

    def so_lambda_energy(self, e_tol=1e-6, l_tol=1e-7):
        return self._so_step(self.L.afesp_ccsd_so_lambda_energy, e_tol, l_tol)

    def so_lambda_diis(self):
        self._chk(self.L.afesp_ccsd_so_lambda_diis(self.h))

    def so_lambda(self):
        o, v = self.so_o, self.so_v
        l1 = np.zeros(o * v)
        l2 = np.zeros(o * o * v * v)
        self._chk(self.L.afesp_ccsd_so_get_lambda(self.h, l1, l2))
        return l1.reshape((o, v), order="F"), l2.reshape((o, o, v, v), order="F")

    def so_set_lambda(self, l1, l2):
        self._chk(self.L.afesp_ccsd_so_set_lambda(self.h, _f(l1), _f(l2)))

    def so_density(self, capacity=None):
        """The symmetrised correlation part of the unrelaxed one-particle density, (o+v) x (o+v) in the state's spin-orbital order"""
        n = self.so_o + self.so_v
        buf = np.zeros(n * n)
        self._chk(self.L.afesp_ccsd_so_density(self.h, buf, buf.size if capacity is None else capacity))
        return buf.reshape((n, n), order="F")

    def so_lambda_t(self, t_begin=0, t_end=None):
        """Lambda-CCSD(T): the triples [t_begin, t_end) of do_ccsd_t_spinorb's list with l1 / l2 in the left factor, at the current t and l
        (needs a live Lambda state: status 21 otherwise).  Writes no amplitude of either kind."""
        if t_end is None:
            t_end = self.so_ntriples()
        e = dbl()
        self._chk(self.L.afesp_ccsd_so_lambda_t(self.h, t_begin, t_end, C.byref(e)))
        return e.value

    def so_eom_t(self, omega, L, R, t_begin=0, t_end=None):
        """The non-iterative triples correction to EOM-EE-CCSD excitation energies: omega[ns], L = [(l1, l2)] and
        R = [(r1, r2)] per state, laid out as t1 / t2 and biorthonormal (afesp_amd.eom.biorthonormalise) -> delta[ns] over the triples
        [t_begin, t_end) of do_ccsd_t_spinorb's list.  All states in one call; writes nothing of the state."""
        if t_end is None:
            t_end = self.so_ntriples()
        omega = np.ascontiguousarray(np.atleast_1d(np.asarray(omega, dtype=np.float64)))
        ns = omega.size
        if len(L) != ns or len(R) != ns:
            raise ValueError("so_eom_t: one left and one right vector per excitation energy")
        cat = lambda vecs, part: np.ascontiguousarray(np.concatenate([_f(x[part]) for x in vecs])) if ns else np.zeros(0)
        l1, l2, r1, r2 = cat(L, 0), cat(L, 1), cat(R, 0), cat(R, 1)
        n1, n2 = self.so_o * self.so_v, (self.so_o * self.so_v) ** 2
        if ns and (l1.size != ns * n1 or r1.size != ns * n1 or l2.size != ns * n2 or r2.size != ns * n2):
            raise ValueError("so_eom_t: vectors are not laid out as t1 / t2 of this state")
        out = np.zeros(max(ns, 1))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.L.afesp_ccsd_so_eom_t(self.h, ns, ptr(omega), ptr(l1), ptr(l2), ptr(r1), ptr(r2), t_begin, t_end, ptr(out)))
        return out[:ns]

    # ---- the two-particle density of the spin-orbital state (include/afesp.h; afesp_amd.density drives them).  All need a
    # live Lambda state; get / energy / expect need a build of the current t and lambda (status 21 otherwise)
    def so_density2_build(self):
        """The correlation part of the two-particle density for the current t and lambda, kept on the device"""
        self._chk(self.L.afesp_ccsd_so_density2_build(self.h))

    def so_density2_shape(self, name):
        o, v = self.so_o, self.so_v
        if name == "vvvv_pairs":
            return (v * (v - 1) // 2,) * 2
        if name == "full":
            return (o + v,) * 4
        if name not in ("oooo", "ooov", "oovv", "ovov", "ovvv", "vvvv"):
            raise ValueError(f"so_density2_get: unknown name {name}")
        return tuple(o if ch == "o" else v for ch in name)

    def so_density2_get(self, name, capacity=None):
        """A stored block (oooo ooov oovv ovov ovvv), the pair matrix vvvv_pairs, or the host-side expansions vvvv and full"""
        dims = self.so_density2_shape(name)
        buf = np.zeros(max(int(np.prod(dims)), 1))
        n = int(np.prod(dims))
        self._chk(self.L.afesp_ccsd_so_density2_get(self.h, name.encode(), buf.ctypes.data_as(C.c_void_p), n if capacity is None else capacity))
        return buf[:n].reshape(dims, order="F")

    def so_density2_energy(self):
        """[sum f D, the six 1/4 sum g Gamma family contributions (oooo ooov oovv ovov ovvv vvvv), their sum]"""
        e = np.zeros(8)
        self._chk(self.L.afesp_ccsd_so_density2_energy(self.h, e.ctypes.data_as(C.c_void_p)))
        return e

    def so_density2_expect(self, a, b):
        """sum_pqrs Gamma_pqrs A_pr B_qs for two (o+v) x (o+v) matrices in the state's spin-orbital order"""
        n = self.so_o + self.so_v
        a, b = _f(a), _f(b)
        if a.size != n * n or b.size != n * n:
            raise ValueError("so_density2_expect: A and B are (o+v) x (o+v)")
        val = dbl()
        self._chk(self.L.afesp_ccsd_so_density2_expect(self.h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(val)))
        return val.value

    # ---- orbital relaxation (include/afesp.h; afesp_amd.density.so_relaxed_density_solve drives them).  All need a build of
    # the two-particle density of the current t and lambda (status 21 otherwise); w, x, y and z are (o, v) arrays laid out as t1
    def so_orbital_gradient(self, fock_response=True, capacity=None):
        """w_ai = dL/dkappa_ai of the Lagrangian on the rotated (f, g); fock_response: f follows the occupied space"""
        o, v = self.so_o, self.so_v
        buf = np.zeros(max(o * v, 1))
        self._chk(self.L.afesp_ccsd_so_orbital_gradient(self.h, int(fock_response), buf.ctypes.data_as(C.c_void_p), o * v if capacity is None else capacity))
        return buf[:o * v].reshape((o, v), order="F")

    def so_zvector_apply(self, x):
        """y = A x, A_ai,bj = delta (e_a - e_i) + <ab||ij> + <aj||ib>"""
        o, v = self.so_o, self.so_v
        x = _f(x)
        if x.size != o * v:
            raise ValueError("so_zvector_apply: x is (o, v)")
        y = np.zeros(max(o * v, 1))
        self._chk(self.L.afesp_ccsd_so_zvector_apply(self.h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)))
        return y[:o * v].reshape((o, v), order="F")

    def so_zvector_solve(self, tol=1e-10, maxiter=100):
        """A z = -w by preconditioned conjugate gradients on the device -> (z, iterations, residual norm).  Status 25 when tol is not
        reached (self.so_zvector_last then holds the iteration count and the residual), 24 on a state made by uso_init_fock"""
        o, v = self.so_o, self.so_v
        z = np.zeros(max(o * v, 1))
        it, res = C.c_int(0), dbl(0.0)
        rc = self.L.afesp_ccsd_so_zvector_solve(self.h, tol, maxiter, z.ctypes.data_as(C.c_void_p), C.byref(it), C.byref(res))
        self.so_zvector_last = (it.value, res.value)
        self._chk(rc)
        return z[:o * v].reshape((o, v), order="F"), it.value, res.value

    def so_relaxed_density(self, capacity=None):
        """The unrelaxed matrix of so_density plus 1/2 z on the ov and vo blocks (needs a converged so_zvector_solve of the current t, lambda)"""
        n = self.so_o + self.so_v
        buf = np.zeros(n * n)
        self._chk(self.L.afesp_ccsd_so_relaxed_density(self.h, buf.ctypes.data_as(C.c_void_p), buf.size if capacity is None else capacity))
        return buf.reshape((n, n), order="F")

    def so_relax_pair_row(self, which, reps=0):
        """Diagnostic (tools/relax_time.py and the tests; not part of the supported interface): the o v^4 term `which` of the orbital gradient
        alone -> (out (o, v), device ms per call over reps calls after a warm one)"""
        o, v = self.so_o, self.so_v
        out = np.zeros(max(o * v, 1))
        ms = dbl(0.0)
        self._chk(self.L.afesp_ccsd_so_relax_pair_row(self.h, which, out.ctypes.data_as(C.c_void_p), reps, C.byref(ms)))
        return out[:o * v].reshape((o, v), order="F"), ms.value

    # ---- The EOM-CCSD eigenproblems of the spin-orbital state (include/afesp.h; afesp_amd.eom drives them): EE, its left-hand side, and
    # the IP and EA sectors.  All need a live Lambda state (so_lambda_init for the current t1 / t2; status 21 otherwise); none writes
    # t1 / t2 or lambda, and no call for one problem touches the state of another.  One set of helpers serves them, keyed by kind:
    # "ee", "left", the sector of the ipea calls -- EOM_IP (1h + 2h1p: r1 (o,), r2 (o,o,v)) or EOM_EA (1p + 2p1h: r1 (v,), r2 (o,v,v)) -- or
    # ("left", sector) for the sector's left-hand side
    EOM_IP, EOM_EA = 1, 2
    _eom_nroots = {}                                                        # kind -> nroots of its last init

    def _eom_shapes(self, kind):
        o, v = self.so_o, self.so_v
        if kind in ("ee", "left"):
            return (o, v), (o, o, v, v)
        sector = kind[1] if isinstance(kind, tuple) else kind
        return ((o,), (o, o, v)) if sector == self.EOM_IP else ((v,), (o, v, v))

    def _eom_fn(self, kind, call):
        """the library's entry `call` of the kind -> (function, its arguments between the context and the call's own)"""
        if kind == "ee":
            return getattr(self.L, "afesp_ccsd_so_eom_" + call), ()
        if kind == "left":
            return getattr(self.L, "afesp_ccsd_so_eom_" + ("lsigma" if call == "sigma" else "left_" + call)), ()
        if isinstance(kind, tuple):
            return getattr(self.L, "afesp_ccsd_so_eom_ipea_" + ("lsigma" if call == "sigma" else "left_" + call)), (kind[1],)
        return getattr(self.L, "afesp_ccsd_so_eom_ipea_" + call), (kind,)

    def _eom_stack(self, kind, x1, x2, who):
        """k vectors with a leading axis, or one vector -> (k, flat x1, flat x2, single)"""
        sh1, sh2 = self._eom_shapes(kind)
        x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
        single = x1.ndim == len(sh1)
        if single:
            x1, x2 = x1[None], x2[None]
        k = x1.shape[0]
        if x1.shape != (k, *sh1) or x2.shape != (k, *sh2):
            raise ValueError(f"{who}: the vectors do not have the shapes (k,) {sh1} / (k,) {sh2} of this state")
        return k, np.concatenate([_f(x) for x in x1]), np.concatenate([_f(x) for x in x2]), single

    def _eom_init(self, kind, nroots, max_space):
        fn, lead = self._eom_fn(kind, "init")
        self._chk(fn(self.h, *lead, nroots, max_space))
        self._eom_nroots = {**self._eom_nroots, kind: int(nroots)}

    def _eom_sigma(self, kind, x1, x2, who):
        sh1, sh2 = self._eom_shapes(kind)
        k, a1, a2, single = self._eom_stack(kind, x1, x2, who)
        s1, s2 = np.zeros_like(a1), np.zeros_like(a2)
        fn, lead = self._eom_fn(kind, "sigma")
        self._chk(fn(self.h, *lead, k, a1, a2, s1, s2))
        s1 = np.stack([x.reshape(sh1, order="F") for x in s1.reshape(k, -1)])
        s2 = np.stack([x.reshape(sh2, order="F") for x in s2.reshape(k, -1)])
        return (s1[0], s2[0]) if single else (s1, s2)

    def _eom_guess(self, kind):
        fn, lead = self._eom_fn(kind, "guess")
        self._chk(fn(self.h, *lead))

    def _eom_set_guess(self, kind, k, x1, x2):
        fn, lead = self._eom_fn(kind, "set_guess")
        self._chk(fn(self.h, *lead, k, _f(x1), _f(x2)))

    def _eom_iterate(self, kind, tol):
        n = self._eom_nroots.get(kind, 1)
        om, rs, fl = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        ns, cv = C.c_int(), C.c_int()
        fn, lead = self._eom_fn(kind, "iterate")
        self._chk(fn(self.h, *lead, tol, om, rs, fl, C.byref(ns), C.byref(cv)))
        return om, rs, fl, ns.value, bool(cv.value)

    def _eom_vector(self, kind, k):
        sh1, sh2 = self._eom_shapes(kind)
        x1, x2 = np.zeros(int(np.prod(sh1))), np.zeros(int(np.prod(sh2)))
        fn, lead = self._eom_fn(kind, "get_vector")
        self._chk(fn(self.h, *lead, k, x1, x2))
        return x1.reshape(sh1, order="F"), x2.reshape(sh2, order="F")

    # EOM-EE-CCSD excitation energies
    def so_eom_init(self, nroots, max_space):
        self._eom_init("ee", nroots, max_space)

    def so_eom_sigma(self, r1, r2):
        """sigma = A r.  r1 (o,v) and r2 (o,o,v,v) for one vector -> (s1, s2); with a leading axis, (k,o,v) and (k,o,o,v,v), k vectors in one
        call -> the same with that axis."""
        return self._eom_sigma("ee", r1, r2, "so_eom_sigma")

    def so_eom_guess(self):
        self._eom_guess("ee")

    def so_eom_set_guess(self, k, r1, r2):
        self._eom_set_guess("ee", k, r1, r2)

    def so_eom_iterate(self, tol=1e-8):
        """One Davidson step -> (omega, resnorm, flags, sigma builds so far, converged); flags: bit 0 converged, bit 1 complex"""
        return self._eom_iterate("ee", tol)

    def so_eom_vector(self, k):
        """Ritz vector k of the last step, <x, x> = sum x1^2 + 1/4 sum x2^2 = 1"""
        return self._eom_vector("ee", k)

    # EOM-EE-CCSD left eigenvectors: the left Davidson state stands beside the right-hand one
    def so_eom_lsigma(self, l1, l2):
        """sigma_L = A^T l.  l1 (o,v) and l2 (o,o,v,v) for one vector -> (s1, s2); with a leading axis, k vectors in one call -> the same
        with that axis."""
        return self._eom_sigma("left", l1, l2, "so_eom_lsigma")

    def so_eom_left_init(self, nroots, max_space):
        self._eom_init("left", nroots, max_space)

    def so_eom_left_guess(self):
        self._eom_guess("left")

    def so_eom_left_set_guess(self, k, l1, l2):
        self._eom_set_guess("left", k, l1, l2)

    def so_eom_left_iterate(self, tol=1e-8):
        """One Davidson step of the left state -> (omega, resnorm, flags, sigma builds so far, converged)"""
        return self._eom_iterate("left", tol)

    def so_eom_left_vector(self, k):
        """Left Ritz vector k of the last step, <x, x> = 1 (biorthonormalise it against the right vectors: afesp_amd.eom)"""
        return self._eom_vector("left", k)

    # EOM-IP-CCSD / EOM-EA-CCSD: sector is EOM_IP or EOM_EA; the rules and statuses are those of the EE calls
    def so_eom_ipea_shapes(self, sector):
        return self._eom_shapes(sector)

    def so_eom_ipea_init(self, sector, nroots, max_space):
        self._eom_init(sector, nroots, max_space)

    def so_eom_ipea_sigma(self, sector, r1, r2):
        """sigma = A r of the sector for one vector -> (s1, s2); with a leading axis, k vectors in one call -> the same with that axis."""
        return self._eom_sigma(sector, r1, r2, "so_eom_ipea_sigma")

    def so_eom_ipea_guess(self, sector):
        self._eom_guess(sector)

    def so_eom_ipea_set_guess(self, sector, k, r1, r2):
        self._eom_set_guess(sector, k, r1, r2)

    def so_eom_ipea_iterate(self, sector, tol=1e-8):
        """One Davidson step of the sector -> (omega, resnorm, flags, sigma builds so far, converged)"""
        return self._eom_iterate(sector, tol)

    def so_eom_ipea_vector(self, sector, k):
        """Ritz vector k of the sector's last step, <x, x> = sum x1^2 + 1/2 sum x2^2 = 1"""
        return self._eom_vector(sector, k)

    # the left-hand side of the sectors: one more Davidson state per sector, for A^T, beside the right-hand one
    def so_eom_ipea_lsigma(self, sector, l1, l2):
        """sigma_L = A^T l of the sector (the transpose in its metric) for one vector -> (s1, s2); with a leading axis, k vectors in one
        call -> the same with that axis."""
        return self._eom_sigma(("left", sector), l1, l2, "so_eom_ipea_lsigma")

    def so_eom_ipea_left_init(self, sector, nroots, max_space):
        self._eom_init(("left", sector), nroots, max_space)

    def so_eom_ipea_left_guess(self, sector):
        self._eom_guess(("left", sector))

    def so_eom_ipea_left_set_guess(self, sector, k, l1, l2):
        self._eom_set_guess(("left", sector), k, l1, l2)

    def so_eom_ipea_left_iterate(self, sector, tol=1e-8):
        """One Davidson step of the sector's left state -> (omega, resnorm, flags, sigma builds so far, converged)"""
        return self._eom_iterate(("left", sector), tol)

    def so_eom_ipea_left_vector(self, sector, k):
        """Left Ritz vector k of the sector's last step, <x, x> = 1 (biorthonormalise it against the right vectors: afesp_amd.eom)"""
        return self._eom_vector(("left", sector), k)

    def so_eom_ipea_dyson(self, sector, l=None, r=None):
        """The Dyson vectors over the o + v spin orbitals of the state (its order) of left vectors l = (l1, l2) and / or right vectors
        r = (r1, r2) of the sector -> (gamma_L, gamma_R), None for an absent side; one vector -> (o+v,), with a leading axis (k, o+v).
        A half-given pair -- (l1, None) -- is passed on and refused by the library."""
        n = self.so_o + self.so_v
        ptrs, outs, keep, k, single = [], [], [], None, True
        for x in (l, r):
            if x is None:
                ptrs += [None, None]
                outs.append(None)
                continue
            if x[0] is None or x[1] is None:                                # half a pair: the library's refusal
                k = k or 1
                a = [None if y is None else _f(y) for y in x]
            else:
                kk, a1, a2, single = self._eom_stack(sector, x[0], x[1], "so_eom_ipea_dyson")
                if k is not None and kk != k and all(p is not None for p in ptrs):
                    raise ValueError("so_eom_ipea_dyson: as many left as right vectors")
                k, a = kk, [a1, a2]
            keep += a
            ptrs += [None if y is None else y.ctypes.data_as(C.c_void_p) for y in a]
            outs.append(np.zeros(n * k))
        if k is None:
            k = 1
        d = [None if y is None else y.ctypes.data_as(C.c_void_p) for y in outs]
        self._chk(self.L.afesp_ccsd_so_eom_ipea_dyson(self.h, sector, k, *ptrs, *d))
        shape = lambda y: None if y is None else (y.copy() if single else y.reshape(k, n))
        return shape(outs[0]), shape(outs[1])

    def so_eom_ipea_t_nitems(self, sector):
        """How many items the sector's triples correction runs over: the triples i<j<k of do_ccsd_t_spinorb's list (IP) or the pairs i<j
        numbered j (j - 1) / 2 + i (EA)"""
        return int(self.L.afesp_ccsd_so_eom_ipea_t_nitems(sector, self.so_o))

    def so_eom_ipea_t(self, sector, omega, L, R, begin=0, end=None):
        """The non-iterative triples correction to EOM-IP-CCSD (sector 1) or EOM-EA-CCSD (sector 2) roots: omega[ns],
        L = [(l1, l2)] and R = [(r1, r2)] per state in the sector's layout, biorthonormal (afesp_amd.eom.biorthonormalise_ipea)
        -> delta[ns] over the items [begin, end).  All states in one call; writes nothing of the state."""
        if end is None:
            end = self.so_eom_ipea_t_nitems(sector)
        omega = np.ascontiguousarray(np.atleast_1d(np.asarray(omega, dtype=np.float64)))
        ns = omega.size
        if len(L) != ns or len(R) != ns:
            raise ValueError("so_eom_ipea_t: one left and one right vector per root")
        cat = lambda vecs, part: np.ascontiguousarray(np.concatenate([_f(x[part]) for x in vecs])) if ns else np.zeros(0)
        l1, l2, r1, r2 = cat(L, 0), cat(L, 1), cat(R, 0), cat(R, 1)
        if sector in (1, 2):
            sh1, sh2 = self._eom_shapes(sector)
            n1, n2 = int(np.prod(sh1)), int(np.prod(sh2))
            if ns and (l1.size != ns * n1 or r1.size != ns * n1 or l2.size != ns * n2 or r2.size != ns * n2):
                raise ValueError(f"so_eom_ipea_t: vectors are not laid out as {sh1} / {sh2} of this state's sector")
        out = np.zeros(max(ns, 1))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.L.afesp_ccsd_so_eom_ipea_t(self.h, sector, ns, ptr(omega), ptr(l1), ptr(l2), ptr(r1), ptr(r2), begin, end, ptr(out)))
        return out[:ns]

    # the reference coupling of right EE vectors and the bilinear density of a left and a right pair: they need the Lambda state only
    def so_eom_ref_coupling(self, r1, r2):
        """c = sum H_ia r_ia + 1/4 sum <ij||ab> r_ijab of one right vector (-> float) or of k vectors (-> array); r0 = c / omega"""
        k, a1, a2, single = self._eom_stack("ee", r1, r2, "so_eom_ref_coupling")
        c = np.zeros(k)
        self._chk(self.L.afesp_ccsd_so_eom_ref_coupling(self.h, k, a1, a2, c))
        return float(c[0]) if single else c

    def so_eom_density(self, l0, l, r0, r, capacity=None):
        """The symmetrised one-particle matrix of <0| (l0 + L) H-bar (r0 + R) |0> over the state's spin orbitals, (o+v) x (o+v).
        l, r: (x1, x2), or None for a zero vector (not read)."""
        o, v, n = self.so_o, self.so_v, self.so_o + self.so_v
        for x in (l, r):
            if x is not None and (np.shape(x[0]) != (o, v) or np.shape(x[1]) != (o, o, v, v)):
                raise ValueError("so_eom_density: a vector does not have the shapes o v / o o v v of this state")
        keep = [None if x is None else (_f(x[0]), _f(x[1])) for x in (l, r)]
        ptr = [(None, None) if x is None else (x[0].ctypes.data, x[1].ctypes.data) for x in keep]
        buf = np.zeros(n * n)
        self._chk(self.L.afesp_ccsd_so_eom_density(self.h, l0, ptr[0][0], ptr[0][1], r0, ptr[1][0], ptr[1][1], buf,
                                                   buf.size if capacity is None else capacity))
        return buf.reshape((n, n), order="F")

    # ---- EOM-CCSD linear response of the spin-orbital state (include/afesp.h; afesp_amd.response drives them).  The response state has a
    # basis of its own: no call here touches t1 / t2, lambda or an EOM state
    RESPONSE_POLE, RESPONSE_NOT_CONVERGED = 26, 27
    response_shape = (0, 0)                                                 # (nop, signed frequencies) of the last so_response_init

    def _so_operators(self, x, who):
        n = self.so_o + self.so_v
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 2
        if single:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (n, n):
            raise ValueError(f"{who}: the operators are (k,) o+v x o+v matrices over the spin orbitals of this state")
        return x.shape[0], np.concatenate([_f(m) for m in x]) if x.shape[0] else np.zeros(0), single

    def so_response_xi(self, x):
        """xi^X = <mu| X-bar |0> of one symmetric operator x (o+v, o+v) -> (xi1 (o,v), xi2 (o,o,v,v)); with a leading axis, k operators in
        one launch -> the same with that axis."""
        o, v = self.so_o, self.so_v
        k, flat, single = self._so_operators(x, "so_response_xi")
        x1, x2 = np.zeros(max(k, 1) * o * v), np.zeros(max(k, 1) * o * o * v * v)
        self._chk(self.L.afesp_ccsd_so_response_xi(self.h, k, flat if k else np.zeros(1), x1, x2))
        x1 = np.stack([m.reshape((o, v), order="F") for m in x1.reshape(k, o * v)])
        x2 = np.stack([m.reshape((o, o, v, v), order="F") for m in x2.reshape(k, o * o * v * v)])
        return (x1[0], x2[0]) if single else (x1, x2)

    def so_response_init(self, x, omega_signed, max_space):
        """The response state of the operators x (k, o+v, o+v) for the signed frequencies omega_signed, on one basis of max_space vectors"""
        k, flat, _ = self._so_operators(x, "so_response_init")
        om = np.ascontiguousarray(np.atleast_1d(omega_signed), dtype=np.float64)
        self._chk(self.L.afesp_ccsd_so_response_init(self.h, k, flat if k else np.zeros(1), om.size, om if om.size else np.zeros(1), max_space))
        self.response_shape = (k, om.size)

    def so_response_iterate(self, tol=1e-8):
        """One step -> (resnorm [signed frequencies, nop], sigma builds so far, converged)"""
        nop, nf = self.response_shape
        rs = np.zeros(max(nop * nf, 1))
        ns, cv = C.c_int(), C.c_int()
        self._chk(self.L.afesp_ccsd_so_response_iterate(self.h, tol, rs, C.byref(ns), C.byref(cv)))
        return rs[:nop * nf].reshape(nf, nop), ns.value, bool(cv.value)

    def so_response_vector(self, iop, ifreq):
        """R^X_iop(omega_signed[ifreq]) of the last step -> (r1, r2)"""
        o, v = self.so_o, self.so_v
        r1, r2 = np.zeros(o * v), np.zeros(o * o * v * v)
        self._chk(self.L.afesp_ccsd_so_response_get_vector(self.h, iop, ifreq, r1, r2))
        return r1.reshape((o, v), order="F"), r2.reshape((o, o, v, v), order="F")

    def so_response_function(self, omegas):
        """<<X_a;X_b>>_omega for every omega of omegas whose +omega and -omega solutions are converged in the state -> (nfreq, nop, nop)"""
        nop = self.response_shape[0]
        om = np.ascontiguousarray(np.atleast_1d(omegas), dtype=np.float64)
        out = np.zeros(max(om.size * nop * nop, 1))
        self._chk(self.L.afesp_ccsd_so_response_function(self.h, om.size, om if om.size else np.zeros(1), out))
        return out[:om.size * nop * nop].reshape(om.size, nop, nop)

    # ---- the same at complex frequencies z = omega + i gamma; so_response_iterate steps either kind of state
    def so_response_init_complex(self, x, z_signed, max_space):
        """The response state of the operators x (k, o+v, o+v) for the complex frequencies z_signed, on one real basis of max_space vectors"""
        k, flat, _ = self._so_operators(x, "so_response_init_complex")
        z = np.atleast_1d(np.asarray(z_signed, dtype=np.complex128))
        pairs = np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).ravel()) if z.size else np.zeros(2)
        self._chk(self.L.afesp_ccsd_so_response_init_complex(self.h, k, flat if k else np.zeros(1), z.size, pairs, max_space))
        self.response_shape = (k, z.size)

    def so_response_vector_complex(self, iop, ifreq):
        """R^X_iop(z_signed[ifreq]) of the last step -> (r1, r2), complex"""
        o, v = self.so_o, self.so_v
        a1, a2, b1, b2 = np.zeros(o * v), np.zeros(o * o * v * v), np.zeros(o * v), np.zeros(o * o * v * v)
        self._chk(self.L.afesp_ccsd_so_response_get_vector_complex(self.h, iop, ifreq, a1, a2, b1, b2))
        return (a1 + 1j * b1).reshape((o, v), order="F"), (a2 + 1j * b2).reshape((o, o, v, v), order="F")

    def so_response_function_complex(self, zs):
        """<<X_a;X_b>>_z for every z of zs whose solutions at z and -z (or -conj z) are converged in the state -> complex (nfreq, nop, nop)"""
        nop = self.response_shape[0]
        z = np.atleast_1d(np.asarray(zs, dtype=np.complex128))
        pairs = np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).ravel()) if z.size else np.zeros(2)
        out = np.zeros(max(2 * z.size * nop * nop, 2))
        self._chk(self.L.afesp_ccsd_so_response_function_complex(self.h, z.size, pairs, out))
        out = out[:2 * z.size * nop * nop]
        return (out[0::2] + 1j * out[1::2]).reshape(z.size, nop, nop)

    def do_ccsd_t_spatial_plain(self, t_begin=0, t_end=None):
        """E[T], E(T) only: what plain CCSD(T)_spatial / CCSD[T]_spatial need (no y, no D sums)."""
        out = np.zeros(2)
        if t_end is None:
            t_end = self.ntriples()
        self._chk(self.L.afesp_ccsd_t_plain(self.h, t_begin, t_end, out))
        return out

    # ---- completely renormalised variants (src/ccsd.f90:2338-2551, :2186-2194)
    def build_cr_intermediates(self):
        self._chk(self.L.afesp_ccsd_cr_intermediates(self.h))

    def do_ccsd_t_spatial_cr(self, t_begin=0, t_end=None):
        out = np.zeros(6)
        if t_end is None:
            t_end = self.ntriples()
        self._chk(self.L.afesp_ccsd_t_cr(self.h, t_begin, t_end, out))
        return out

    # ---- src/linalg.fpp operator layer
    def gemm(self, transA, transB, m, n, k, A, B, Cmat=None, alpha=1.0, beta=0.0):
        Cflat = np.zeros(m * n) if Cmat is None else _f(Cmat)
        self._chk(self.L.afesp_gemm(self.h, transA.encode(), transB.encode(), m, n, k, alpha, _f(A), _f(B), beta, Cflat))
        return Cflat.reshape((m, n), order="F")

    def omp_reshape(self, in_arr, order, out_arr=None, beta=None):
        dims = (i64 * 4)(*in_arr.shape)
        oshape = tuple(in_arr.shape[int(ch) - 1] for ch in order)
        out = np.zeros(int(np.prod(oshape))) if out_arr is None else _f(out_arr)
        self._chk(self.L.afesp_permute4(self.h, dims, order.encode(), _f(in_arr), out, 0 if beta is None else 1,
                                        0.0 if beta is None else beta))
        return out.reshape(oshape, order="F")

    def contract(self, alpha, A, la, B, lb, beta, Cmat, lc, force_split=0, force_tm=0, force_tn=0):
        dA, dB, dC = (i64 * len(la))(*A.shape), (i64 * len(lb))(*B.shape), (i64 * len(lc))(*Cmat.shape)
        Cflat = _f(Cmat)
        self._chk(self.L.afesp_contract(self.h, alpha, _f(A), la.encode(), dA, _f(B), lb.encode(), dB, beta, Cflat,
                                        lc.encode(), dC, force_split, force_tm, force_tn))
        return Cflat.reshape(Cmat.shape, order="F")

    def bench_contract(self, la, dA, lb, dB, lc, dC, reps=5):
        ms = dbl()
        self._chk(self.L.afesp_bench_contract(self.h, la.encode(), (i64 * len(dA))(*dA), lb.encode(), (i64 * len(dB))(*dB),
                                              lc.encode(), (i64 * len(dC))(*dC), reps, C.byref(ms)))
        return ms.value

    def profile(self, enable):
        out = np.zeros(8)
        self._chk(self.L.afesp_profile(self.h, 1 if enable else 0, out))
        return dict(gemm_ms=out[0], gemm_launches=int(out[1]), gemm_flop=out[2], orbit_ms=out[3], orbit_launches=int(out[4]),
                    orbit_bytes=out[5], gemm_flop_padded=out[6], gemm_kernel="tgemm_kernel" if out[7] else "gett_kernel")

    def bench_stream(self, n, reps=5):
        ms = dbl()
        self._chk(self.L.afesp_bench_stream(self.h, n, reps, C.byref(ms)))
        return ms.value

    def set_tuning(self, group_m=0, tm=0, tn=0, split=0):
        self.L.afesp_set_tuning(group_m, tm, tn, split)

    def synthetic_ao(self, nbasis, scale=0.02, seed=12345):
        self._chk(self.L.afesp_synthetic_ao(self.h, nbasis, scale, seed))

    def pp_ladder_flop(self):
        f = dbl()
        self._chk(self.L.afesp_ccsd_pp_ladder_flop(self.h, C.byref(f)))
        return f.value

    def iteration_flop(self):
        f = dbl()
        self._chk(self.L.afesp_ccsd_iteration_flop(self.h, C.byref(f)))
        return f.value

    def time_pp_ladder(self, reps=10):
        ms = dbl()
        self._chk(self.L.afesp_time_pp_ladder(self.h, reps, C.byref(ms)))
        return ms.value
