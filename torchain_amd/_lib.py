"""ctypes binding of libtorchain_hip.so, the C-ABI drop-in boundary (include/torchain_hip.h).

The reference binds its C functions through cffi (``torchain/functions.py:5-6``,
``build.py:19-31``); here the same role is played by ctypes on a hipcc-built shared library that
takes raw device pointers.  There is no CPU fallback: if the library is missing the import of this
module raises, and every hot call requires CUDA/ROCm tensors.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtorchain_hip.so")

TC_OK = 0
TC_DTYPE_F32, TC_DTYPE_BF16, TC_DTYPE_F16 = 0, 1, 2  # element types of tc_chain_step_typed
TC_LAYOUT_ROWS, TC_LAYOUT_BCT, TC_LAYOUT_CHANNEL_LAST = 0, 1, 2  # layouts of tc_chain_step_strided
ERRORS = {
    -1: "TC_ERR_INVALID_ARGUMENT", -2: "TC_ERR_BAD_FST", -3: "TC_ERR_UNSUPPORTED", -4: "TC_ERR_WORKSPACE",
    -5: "TC_ERR_HIP", -6: "TC_ERR_IO", -7: "TC_ERR_NOT_SEPARABLE",
}


class TorchainHipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib.tc_strerror(code).decode() if _lib is not None else "?"
        extra = " (hipError %d)" % lib.tc_last_hip_error() if code == -5 else ""
        super().__init__("%s failed: %s [%s]%s" % (where, msg, ERRORS.get(code, code), extra))


_lib = None


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "torchain_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C torchain_amd/csrc`; there is no CPU fallback for the chain loss." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.tc_strerror.restype = C.c_char_p
    L.tc_strerror.argtypes = [C.c_int]
    L.tc_version.restype = C.c_int
    L.tc_last_hip_error.restype = C.c_int
    L.tc_den_graph_create.restype = C.c_int
    L.tc_den_graph_create.argtypes = [C.POINTER(vp), i32, i64, vp, vp, vp, vp, vp, i32, i32]
    L.tc_den_graph_read.restype = C.c_int
    L.tc_den_graph_read.argtypes = [C.POINTER(vp), C.c_char_p, i32]
    L.tc_den_graph_free.restype = None
    L.tc_den_graph_free.argtypes = [vp]
    L.tc_den_graph_num_states.restype = i32
    L.tc_den_graph_num_states.argtypes = [vp]
    L.tc_den_graph_num_arcs.restype = i64
    L.tc_den_graph_num_arcs.argtypes = [vp]
    L.tc_den_graph_num_pdfs.restype = i32
    L.tc_den_graph_num_pdfs.argtypes = [vp]
    L.tc_den_graph_initial_probs.restype = C.c_int
    L.tc_den_graph_initial_probs.argtypes = [vp, vp]
    L.tc_supervision_append.restype = C.c_int
    L.tc_supervision_append.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp]
    L.tc_self_test.restype = C.c_int
    L.tc_self_test.argtypes = [C.c_int, vp, vp]
    L.tc_den_graph_prepare.restype = C.c_int
    L.tc_den_graph_prepare.argtypes = [vp, C.c_int]
    L.tc_den_graph_stats.restype = C.c_int
    L.tc_den_graph_stats.argtypes = [vp, vp]
    L.tc_example_read.restype = C.c_int
    L.tc_example_read.argtypes = [vp, vp, C.c_int32, C.c_int, vp]
    L.tc_archive_open.restype = C.c_int
    L.tc_archive_open.argtypes = [C.c_char_p, vp]
    L.tc_archive_next.restype = C.c_int
    L.tc_archive_next.argtypes = [vp, vp, C.c_int32, vp]
    L.tc_archive_close.restype = C.c_int
    L.tc_archive_close.argtypes = [vp]
    L.tc_example_free.restype = None
    L.tc_example_free.argtypes = [vp]
    L.tc_example_last_error.restype = C.c_char_p
    L.tc_example_last_error.argtypes = []
    L.tc_example_counts.restype = C.c_int
    L.tc_example_counts.argtypes = [vp, vp]
    L.tc_example_input.restype = C.c_int
    L.tc_example_input.argtypes = [vp, C.c_int32] + [vp] * 6
    L.tc_example_output.restype = C.c_int
    L.tc_example_output.argtypes = [vp, C.c_int32] + [vp] * 11
    L.tc_den_graph_tuning.restype = C.c_int
    L.tc_den_graph_tuning.argtypes = [vp, C.c_int, vp, vp, vp]
    L.tc_den_graph_set_variant.restype = C.c_int
    L.tc_den_graph_set_variant.argtypes = [vp, C.c_int, C.c_int32]
    L.tc_den_graph_hash.restype = C.c_uint64
    L.tc_den_graph_hash.argtypes = [vp]
    L.tc_tuning_cache_get.restype = C.c_int
    L.tc_tuning_cache_get.argtypes = [C.c_uint64, C.c_char_p, C.POINTER(C.c_int32)]
    L.tc_tuning_cache_put.restype = C.c_int
    L.tc_tuning_cache_put.argtypes = [C.c_uint64, C.c_char_p, C.c_int32, C.c_float, C.c_float]
    L.tc_debug_set.restype = C.c_int
    L.tc_debug_set.argtypes = [C.c_char_p, C.c_int]
    L.tc_debug_counter.restype = C.c_int64
    L.tc_debug_counter.argtypes = [C.c_char_p]
    L.tc_den_graph_debug_walk.restype = C.c_int
    L.tc_den_graph_debug_walk.argtypes = [vp, C.c_int, vp, vp, vp]
    L.tc_to2d.restype = C.c_int
    L.tc_to2d.argtypes = [vp, i32, i32, i32, vp, i64, C.c_int, vp]
    L.tc_from2d.restype = C.c_int
    L.tc_from2d.argtypes = [vp, i64, i32, i32, i32, f32, vp, C.c_int, vp]
    L.tc_supervision_create.restype = C.c_int
    L.tc_supervision_create.argtypes = [C.POINTER(vp), f32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.tc_supervision_create_e2e.restype = C.c_int
    L.tc_supervision_create_e2e.argtypes = [C.POINTER(vp), f32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.tc_supervision_is_e2e.restype = i32
    L.tc_supervision_is_e2e.argtypes = [vp]
    L.tc_supervision_create_e2e_ragged.restype = C.c_int
    L.tc_supervision_create_e2e_ragged.argtypes = [C.POINTER(vp), f32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.tc_supervision_create_e2e_any.restype = C.c_int
    L.tc_supervision_create_e2e_any.argtypes = [C.POINTER(vp), f32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.tc_supervision_e2e_stats.restype = C.c_int
    L.tc_supervision_e2e_stats.argtypes = [vp, vp]
    L.tc_supervision_create_ragged.restype = C.c_int
    L.tc_supervision_create_ragged.argtypes = [C.POINTER(vp), f32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.tc_supervision_frames.restype = C.c_int
    L.tc_supervision_frames.argtypes = [vp, vp]
    L.tc_supervision_is_ragged.restype = i32
    L.tc_supervision_is_ragged.argtypes = [vp]
    L.tc_example_output_e2e.restype = C.c_int
    L.tc_example_output_e2e.argtypes = [vp, C.c_int32, vp, vp, vp]
    L.tc_rand_reader_new.restype = C.c_int
    L.tc_rand_reader_new.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, vp]
    L.tc_rand_reader_new_ordered.restype = C.c_int
    L.tc_rand_reader_new_ordered.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    for name in ("tc_rand_reader_reset", "tc_rand_reader_num_batch", "tc_rand_reader_num_data", "tc_rand_reader_next"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp]
    for name in ("tc_rand_reader_example", "tc_rand_reader_supervision_new", "tc_rand_reader_take_example"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp, vp]
    L.tc_rand_reader_set_device.restype = C.c_int
    L.tc_rand_reader_set_device.argtypes = [vp, C.c_int]
    L.tc_supervision_stage.restype = C.c_int
    L.tc_supervision_stage.argtypes = [vp, C.c_int]
    L.tc_rand_reader_batch_keys.restype = C.c_int
    L.tc_rand_reader_batch_keys.argtypes = [vp, C.c_int32, C.c_char_p, C.c_int32]
    L.tc_rand_reader_free.restype = None
    L.tc_rand_reader_free.argtypes = [vp]
    L.tc_rand_reader_last_error.restype = C.c_char_p
    L.tc_rand_reader_last_error.argtypes = []
    L.tc_chain_step_workspace_bytes.restype = C.c_int64
    L.tc_chain_step_workspace_bytes.argtypes = [vp, C.c_int32, C.c_int32, C.c_int, C.c_int]
    L.tc_chain_step.restype = C.c_int
    L.tc_chain_step.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp,
                                vp, vp, C.c_int64, C.c_int, vp]
    L.tc_chain_step_typed_workspace_bytes.restype = C.c_int64
    L.tc_chain_step_typed_workspace_bytes.argtypes = [vp, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_int]
    L.tc_chain_step_typed.restype = C.c_int
    L.tc_chain_step_typed.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, vp, vp,
                                      vp, vp, vp, C.c_int, vp, C.c_int64, C.c_int, vp]
    L.tc_chain_step_weighted.restype = C.c_int
    L.tc_chain_step_weighted.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, vp,
                                         vp, vp, vp, vp, vp, C.c_int, vp, C.c_int64, C.c_int, vp]
    L.tc_chain_step_penalized.restype = C.c_int
    L.tc_chain_step_penalized.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int, vp,
                                          vp, vp, vp, vp, vp, C.c_float, C.c_int, vp, C.c_int64, C.c_int, vp]
    L.tc_chain_step_strided_workspace_bytes.restype = C.c_int64
    L.tc_chain_step_strided_workspace_bytes.argtypes = [vp, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_int]
    L.tc_chain_step_strided.restype = C.c_int
    L.tc_chain_step_strided.argtypes = [vp, vp, vp, vp, C.c_int, i64, i64, i64, C.c_float, C.c_float, C.c_float, C.c_int, vp,
                                        vp, vp, vp, vp, vp, C.c_float, C.c_int, vp, C.c_int64, C.c_int, vp]
    L.tc_chain_step_per_sequence.restype = C.c_int
    L.tc_chain_step_per_sequence.argtypes = L.tc_chain_step_strided.argtypes + [C.c_int, vp]
    L.tc_chain_step_log_softmax_workspace_bytes.restype = C.c_int64
    L.tc_chain_step_log_softmax_workspace_bytes.argtypes = L.tc_chain_step_strided_workspace_bytes.argtypes
    L.tc_chain_step_log_softmax.restype = C.c_int
    L.tc_chain_step_log_softmax.argtypes = L.tc_chain_step_per_sequence.argtypes + [C.c_int]
    L.tc_chain_step_boosted_workspace_bytes.restype = C.c_int64
    L.tc_chain_step_boosted_workspace_bytes.argtypes = L.tc_chain_step_strided_workspace_bytes.argtypes
    L.tc_chain_step_boosted.restype = C.c_int
    L.tc_chain_step_boosted.argtypes = L.tc_chain_step_log_softmax.argtypes + [f32, vp, vp, vp, i64]
    L.tc_boost_rows.restype = C.c_int
    L.tc_boost_rows.argtypes = [vp, C.c_int, C.c_int, i32, i32, i32, i64, i64, i64, vp, f32, vp, vp, vp, i64, vp, i64, C.c_int, vp]
    L.tc_rows_gather.restype = C.c_int
    L.tc_rows_gather.argtypes = [vp, C.c_int, i32, i32, i32, i64, i64, vp, i64, C.c_int, vp]
    L.tc_rows_scatter.restype = C.c_int
    L.tc_rows_scatter.argtypes = [vp, i64, C.c_int, i32, i32, i32, f32, vp, f32, vp, i64, i64, vp, C.c_int, vp]
    L.tc_supervision_free.restype = None
    L.tc_supervision_free.argtypes = [vp]
    for name in ("tc_supervision_num_pdf", "tc_supervision_num_sequence", "tc_supervision_num_frame"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp]
    L.tc_supervision_weight.restype = f32
    L.tc_supervision_weight.argtypes = [vp]
    L.tc_supervision_stats.restype = C.c_int
    L.tc_supervision_stats.argtypes = [vp, vp]
    L.tc_supervision_prepare.restype = C.c_int
    L.tc_supervision_prepare.argtypes = [vp, C.c_int, vp]
    L.tc_chain_workspace_bytes.restype = i64
    L.tc_chain_workspace_bytes.argtypes = [vp, i32, i32]
    L.tc_chain_objf_and_deriv.restype = C.c_int
    L.tc_chain_objf_and_deriv.argtypes = [vp, vp, vp, i64, i32, i64, vp, vp, i64, vp, i64, f32, f32, f32, vp, i64,
                                          C.c_int, vp]
    L.tc_chain_objf_and_grad.restype = C.c_int
    L.tc_chain_objf_and_grad.argtypes = L.tc_chain_objf_and_deriv.argtypes
    L.tc_den_forward_backward.restype = C.c_int
    L.tc_den_forward_backward.argtypes = [vp, i32, vp, i64, i32, i64, f32, f32, f32, C.c_int, vp, i64, vp, vp, vp,
                                          i64, C.c_int, vp]
    L.tc_den_forward_backward_ragged.restype = C.c_int
    L.tc_den_forward_backward_ragged.argtypes = [vp, i32, vp, i64, i32, i64, f32, f32, f32, C.c_int, vp, i64, vp, i32, vp, vp,
                                                 vp, i64, C.c_int, vp]
    L.tc_xent_objf.restype = C.c_int
    L.tc_xent_objf.argtypes = [vp, i64, i32, i64, vp, i64, vp, vp, i64, C.c_int, vp]
    L.tc_num_forward_backward.restype = C.c_int
    L.tc_num_forward_backward.argtypes = [vp, vp, i64, i32, i64, vp, i64, vp, vp, i64, C.c_int, vp]
    L.tc_supervision_best_path.restype = C.c_int
    L.tc_supervision_best_path.argtypes = [vp, vp, C.c_int, C.c_int, i64, i32, i64, vp, vp, C.c_int, vp]
    L.tc_den_best_path_workspace_bytes.restype = i64
    L.tc_den_best_path_workspace_bytes.argtypes = [vp, i32, i32]
    L.tc_den_best_path.restype = C.c_int
    L.tc_den_best_path.argtypes = [vp, i32, vp, C.c_int, C.c_int, i64, i32, i64, vp, i32, vp, vp, vp, vp, i64, C.c_int, vp]
    L.tc_den_expected_accuracy_workspace_bytes.restype = i64
    L.tc_den_expected_accuracy_workspace_bytes.argtypes = [vp, i32, i32]
    L.tc_den_expected_accuracy.restype = C.c_int
    L.tc_den_expected_accuracy.argtypes = [vp, i32, vp, i64, i32, i64, vp, i32, f32, vp, vp, vp, i64, vp, vp, vp, i64,
                                           C.c_int, vp]
    L.tc_den_expected_accuracy_grad_workspace_bytes.restype = i64
    L.tc_den_expected_accuracy_grad_workspace_bytes.argtypes = [vp, i32, i32]
    L.tc_den_expected_accuracy_grad.restype = C.c_int
    L.tc_den_expected_accuracy_grad.argtypes = [vp, i32, vp, i64, i32, i64, vp, i32, f32, vp, vp, vp, vp, vp, i64, vp, i64,
                                                C.c_int, vp]
    L.tc_den_expected_accuracy_dense.restype = C.c_int
    L.tc_den_expected_accuracy_dense.argtypes = [vp, i32, vp, i64, i32, i64, vp, i32, f32, vp, i64, vp, i64, vp, vp, vp, i64,
                                                 C.c_int, vp]
    L.tc_den_expected_accuracy_dense_grad.restype = C.c_int
    L.tc_den_expected_accuracy_dense_grad.argtypes = [vp, i32, vp, i64, i32, i64, vp, i32, f32, vp, i64, vp, vp, vp, i64, vp, i64,
                                                      C.c_int, vp]
    L.tc_den_sample_paths_workspace_bytes.restype = i64
    L.tc_den_sample_paths_workspace_bytes.argtypes = [vp, i32, i32]
    L.tc_den_sample_paths.restype = C.c_int
    L.tc_den_sample_paths.argtypes = [vp, i32, vp, i64, i32, i64, vp, i32, f32, i32, vp, vp, vp, vp, i64, C.c_int, vp]
    L.tc_paths_edit_distance_workspace_bytes.restype = i64
    L.tc_paths_edit_distance_workspace_bytes.argtypes = [i32, i32, i32]
    L.tc_paths_edit_distance.restype = C.c_int
    L.tc_paths_edit_distance.argtypes = [i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i64, C.c_int, vp]
    L.tc_sampled_risk_grad.restype = C.c_int
    L.tc_sampled_risk_grad.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_int, i64, i64, i64, vp, i64, i64, i64, i64,
                                       C.c_int, vp]
    L.tc_den_graph_arcs.restype = C.c_int
    L.tc_den_graph_arcs.argtypes = [vp, vp, vp, vp, vp]
    L.tc_den_compose.restype = C.c_int
    L.tc_den_compose.argtypes = [C.POINTER(vp), vp, i32, i32, C.c_int, vp, vp, vp, vp, vp, vp, vp, f32, i64]
    L.tc_den_compose_sizes.restype = C.c_int
    L.tc_den_compose_sizes.argtypes = [vp, vp]
    L.tc_den_compose_info.restype = C.c_int
    L.tc_den_compose_info.argtypes = [vp, vp, vp]
    L.tc_den_compose_copy.restype = C.c_int
    L.tc_den_compose_copy.argtypes = [vp] * 8
    L.tc_den_compose_free.restype = None
    L.tc_den_compose_free.argtypes = [vp]
    return L


lib = _load()
_lib = lib


def check(code, where):
    if code != TC_OK:
        raise TorchainHipError(code, where)
