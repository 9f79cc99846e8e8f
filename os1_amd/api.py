"""ctypes binding of liborbfe.so (include/orbfe.h).  Mirrors the reference's operator interface:
Extractor(...)(image) ~ ORBextractor::operator(), Matcher.search_for_initialization(...) ~
ORBmatcher::SearchForInitialization, Matcher.search_by_projection(...) ~ SearchByProjection.
No compute happens in Python and there is no fallback: if the library or a GPU is missing the
constructors raise."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get('ORBFE_LIB') or os.path.join(_HERE, 'liborbfe.so')   # ORBFE_LIB: an A/B build of the library (developer aid)

KP_DTYPE = np.dtype([('x', 'f4'), ('y', 'f4'), ('size', 'f4'), ('angle', 'f4'), ('response', 'f4'),
                     ('octave', 'i4'), ('class_id', 'i4')])

MP_IN_VIEW, MP_BAD, MP_CANDIDATO, MP_OBSERVED = 1, 2, 4, 8


class OrbfeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('orbfe error %d: %s' % (code, msg))
        self.code = code


def lib_path():
    return _SO


def build_library(force=False):
    """Compile liborbfe.so for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ['make', '-s', '-C', os.path.join(_HERE, 'csrc')]
    if force:
        subprocess.check_call(args + ['clean'])
    subprocess.check_call(args)
    return _SO


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise OrbfeError(-2, 'liborbfe.so is not built (run __graft_entry__.build() or make -C os1_amd/csrc)')
    L = C.CDLL(_SO)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.orbfe_last_error.restype = C.c_char_p
    L.orbfe_device_count.restype = ci
    L.orbfe_extractor_create.argtypes = [ci, cf, ci, ci, ci, ci, C.POINTER(vp)]
    L.orbfe_extractor_destroy.argtypes = [vp]
    L.orbfe_extractor_destroy.restype = None
    L.orbfe_extractor_levels.argtypes = [vp]
    L.orbfe_extractor_scale_factor.argtypes = [vp]
    L.orbfe_extractor_scale_factor.restype = cf
    L.orbfe_extractor_scale_tables.argtypes = [vp, vp, vp, vp, vp]
    L.orbfe_extractor_features_per_level.argtypes = [vp, vp]
    L.orbfe_extractor_max_keypoints.argtypes = [vp]
    L.orbfe_extract.argtypes = [vp, vp, ci, ci, C.c_size_t, vp, vp, ci, C.POINTER(ci)]
    L.orbfe_extract_batch.argtypes = [vp, ci, vp, ci, ci, ci, C.c_size_t, vp, vp, ci, vp]
    L.orbfe_extract_batch_submit.argtypes = [vp, ci, vp, ci, ci, ci, C.c_size_t]
    L.orbfe_extract_batch_wait.argtypes = [vp]
    L.orbfe_extract_batch_collect.argtypes = [vp, vp, vp, ci, vp]
    L.orbfe_debug_level_size.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci)]
    L.orbfe_debug_level_copy.argtypes = [vp, ci, ci, vp]
    L.orbfe_debug_candidates.argtypes = [vp, ci, ci, vp, ci, C.POINTER(ci)]
    L.orbfe_debug_stage_ms.argtypes = [vp, vp]
    L.orbfe_debug_sincos.argtypes = [vp, vp, ci, vp, vp]
    L.orbfe_hamming.argtypes = [vp, vp]
    L.orbfe_matcher_create.argtypes = [ci, C.POINTER(vp)]
    L.orbfe_matcher_destroy.argtypes = [vp]
    L.orbfe_matcher_destroy.restype = None
    L.orbfe_search_for_initialization.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, ci, cf, ci, C.POINTER(ci)]
    L.orbfe_search_for_initialization_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, cf, ci, vp]
    L.orbfe_frame_create.argtypes = [vp, vp, vp, ci, vp, C.POINTER(vp)]
    L.orbfe_frame_create_from_extract.argtypes = [vp, ci, vp, vp, C.POINTER(vp)]
    L.orbfe_frame_destroy.argtypes = [vp]
    L.orbfe_frame_destroy.restype = None
    L.orbfe_frame_size.argtypes = [vp]
    L.orbfe_frame_descriptors_device.argtypes = [vp]
    L.orbfe_frame_descriptors_device.restype = vp
    L.orbfe_frame_download.argtypes = [vp, vp, vp, vp, vp]
    L.orbfe_search_by_projection_frame.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp, C.POINTER(ci)]
    L.orbfe_search_by_projection_frame_rows.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, cf, cf, vp,
                                                        C.POINTER(ci)]
    L.orbfe_matcher_upload_async.argtypes = [vp, vp, vp, C.c_size_t]
    L.orbfe_matcher_synchronize.argtypes = [vp]
    L.orbfe_matcher_device.argtypes = [vp]
    L.orbfe_extractor_device.argtypes = [vp]
    L.orbfe_frame_device.argtypes = [vp]
    L.orbfe_resident_epoch.restype = C.c_ulonglong
    L.orbfe_resident_invalidate.restype = C.c_ulonglong
    L.orbfe_search_by_projection_uv_frame.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, cf, ci, ci, ci, vp,
                                                      C.POINTER(ci)]
    L.orbfe_search_projected_frame.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, ci, C.c_double, ci, vp, vp,
                                               C.POINTER(ci)]
    L.orbfe_debug_resolve_rounds.argtypes = [vp]
    L.orbfe_debug_resolve_route.argtypes = [vp]
    L.orbfe_debug_resolve_phases.argtypes = [vp, vp]
    L.orbfe_search_by_projection.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp,
                                             C.POINTER(ci)]
    L.orbfe_search_by_projection_uv.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, cf, ci,
                                                ci, ci, vp, C.POINTER(ci)]
    L.orbfe_distinctive_descriptors.argtypes = [vp, ci, vp, vp, vp]
    L.orbfe_window_candidates.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t,
                                          C.POINTER(C.c_size_t)]
    L.orbfe_undistort_equidistant.argtypes = [vp, ci, cf, cf, cf, cf]
    L.orbfe_undistort_pinhole.argtypes = [vp, ci, cf, cf, cf, cf, vp, ci]
    L.orbfe_compute_image_bounds.argtypes = [ci, ci, ci, cf, cf, cf, cf, vp, ci, vp]
    L.orbfe_search_projected.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, ci, C.c_double, ci, vp, vp,
                                         C.POINTER(ci)]
    L.orbfe_search_for_triangulation.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, cf, cf,
                                                 vp, vp, ci, ci, vp, C.POINTER(ci)]
    L.orbfe_search_for_triangulation_frames_batch.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp]
    L.orbfe_triangulation_finish.argtypes = [vp, ci, vp, vp, ci, vp, vp, ci, vp, C.POINTER(ci)]
    L.orbfe_search_for_triangulation_frames.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, C.POINTER(ci)]
    L.orbfe_extractor_max_keypoints_for_size.argtypes = [vp, ci, ci]
    L.orbfe_extractor_set_vocabulary.argtypes = [vp, vp, ci]
    L.orbfe_extract_bow_raw.argtypes = [vp, ci, vp, vp, ci, C.POINTER(ci)]
    L.orbfe_bow_assemble.argtypes = [vp, vp, vp, ci, vp, vp, C.POINTER(ci), vp, vp, vp, C.POINTER(ci), vp]
    L.orbfe_stream_set_vocabulary.argtypes = [vp, vp, ci]
    L.orbfe_stream_bow_raw.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(ci)]
    L.orbfe_extract_bow.argtypes = [vp, ci, vp, vp, C.POINTER(ci), vp, vp, vp, C.POINTER(ci), vp, vp]
    L.orbfe_extractor_set_input_format.argtypes = [vp, ci, ci]
    L.orbfe_stream_set_input_format.argtypes = [vp, ci, ci]
    L.orbfe_extractor_set_blur_variant.argtypes = [vp, ci]
    L.orbfe_extractor_set_camera.argtypes = [vp, ci, cf, cf, cf, cf, vp, ci]
    L.orbfe_extractor_undistort.argtypes = [vp, vp, ci]
    L.orbfe_extractor_set_camera_equidistant.argtypes = [vp, cf, cf, cf, cf]
    L.orbfe_extractor_undistort_verdict.argtypes = [vp, vp, ci, vp, vp]
    L.orbfe_extractor_equidistant_stats.argtypes = [vp, vp]
    L.orbfe_stream_set_camera_equidistant.argtypes = [vp, cf, cf, cf, cf]
    L.orbfe_stream_equidistant_stats.argtypes = [vp, vp]
    L.orbfe_stream_multi_set_camera_equidistant.argtypes = [vp, cf, cf, cf, cf]
    L.orbfe_stream_multi_equidistant_stats.argtypes = [vp, vp]
    L.orbfe_stream_set_camera.argtypes = [vp, ci, cf, cf, cf, cf, vp, ci]
    L.orbfe_stream_xy_un.argtypes = [vp, C.POINTER(vp)]
    L.orbfe_stream_multi_set_camera.argtypes = [vp, ci, cf, cf, cf, cf, vp, ci]
    L.orbfe_stream_multi_xy_un.argtypes = [vp, C.POINTER(vp)]
    L.orbfe_sfi_chain_create.argtypes = [vp, C.POINTER(vp)]
    L.orbfe_sfi_chain_destroy.argtypes = [vp]
    L.orbfe_sfi_chain_destroy.restype = None
    L.orbfe_extract_batch_submit_matched.argtypes = [vp, vp, ci, vp, ci, ci, ci, C.c_size_t, vp, ci, cf, ci]
    L.orbfe_extract_undistorted.argtypes = [vp, vp, ci, ci, C.c_size_t, vp, vp, ci, C.POINTER(ci), vp]
    L.orbfe_extract_batch_collect_undistorted.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_stream_set_blur_variant.argtypes = [vp, ci]
    L.orbfe_vocabulary_create.argtypes = [ci, ci, ci, ci, ci, vp, ci, C.POINTER(vp)]
    L.orbfe_vocabulary_create_from_image.argtypes = [ci, vp, C.c_size_t, C.POINTER(vp)]
    L.orbfe_vocabulary_destroy.argtypes = [vp]
    L.orbfe_vocabulary_destroy.restype = None
    L.orbfe_vocabulary_info.argtypes = [vp] + [C.POINTER(ci)] * 6
    L.orbfe_bow_transform.argtypes = [vp, vp, ci, ci, ci, vp, vp, C.POINTER(ci), vp, vp, vp, C.POINTER(ci), vp, vp]
    L.orbfe_kfdb_create.argtypes = [ci, ci, ci, ci, ci, C.POINTER(vp)]
    L.orbfe_kfdb_destroy.argtypes = [vp]
    L.orbfe_kfdb_destroy.restype = None
    L.orbfe_kfdb_add.argtypes = [vp, C.c_uint64, vp, vp, ci]
    L.orbfe_kfdb_add_batch.argtypes = [vp, ci, vp, vp, vp, vp]
    L.orbfe_bow_transform_batch.argtypes = [vp, ci, ci] + [vp] * 12
    L.orbfe_kfdb_erase.argtypes = [vp, C.c_uint64]
    L.orbfe_kfdb_clear.argtypes = [vp]
    L.orbfe_kfdb_size.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.orbfe_kfdb_query.argtypes = [vp, vp, vp, ci, vp, vp, vp, ci, C.POINTER(ci)]
    L.orbfe_kfdb_score.argtypes = [vp, vp, vp, ci, vp, ci, vp]
    tail = [cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]   # sigma, n_hyp, H21, H12, F21, eight outputs
    L.orbfe_score_init_hypotheses.argtypes = [vp, vp, ci] + tail
    L.orbfe_score_init_hypotheses_kps.argtypes = [vp, vp, ci, vp, ci, vp] + tail + [C.POINTER(ci)]
    L.orbfe_score_init_hypotheses_frames.argtypes = [vp, vp, vp, vp] + tail + [C.POINTER(ci)]
    L.orbfe_score_sim3_hypotheses.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_score_pnp_hypotheses.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_ransac_mask_words.argtypes = [ci, vp, ci, vp]
    L.orbfe_ransac_mask_words.restype = C.c_size_t
    L.orbfe_search_by_bow.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, cf, ci, ci, vp,
                                      C.POINTER(ci)]
    L.orbfe_search_by_bow_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, cf, ci, ci, vp, vp]
    L.orbfe_debug_matcher_ms.argtypes = [vp, vp]
    L.orbfe_debug_features_in_area.argtypes = [vp, vp, ci, vp, cf, cf, cf, ci, ci, vp, ci, C.POINTER(ci)]
    L.orbfe_debug_kernel_ms.argtypes = [vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), ci]
    L.orbfe_debug_set_profiling.argtypes = [vp, ci]
    L.orbfe_device_malloc.argtypes = [ci, C.c_size_t, C.POINTER(vp)]
    L.orbfe_device_free.argtypes = [ci, vp]
    L.orbfe_device_upload.argtypes = [ci, vp, vp, C.c_size_t]
    L.orbfe_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.orbfe_host_free.argtypes = [vp]
    L.orbfe_host_register.argtypes = [vp, C.c_size_t]
    L.orbfe_host_unregister.argtypes = [vp]
    L.orbfe_device_synchronize.argtypes = [ci]
    L.orbfe_device_numa_node.argtypes = [ci]
    L.orbfe_bind_thread_to_device.argtypes = [ci]
    L.orbfe_debug_h2d_rate.argtypes = [ci, vp, C.c_size_t, ci, C.POINTER(C.c_double)]
    L.orbfe_stream_create.argtypes = [ci, cf, ci, ci, ci, ci, ci, ci, C.POINTER(vp)]
    L.orbfe_stream_destroy.argtypes = [vp]
    L.orbfe_stream_destroy.restype = None
    L.orbfe_stream_set_matching.argtypes = [vp, vp, ci, cf, ci]
    L.orbfe_stream_capacity.argtypes = [vp]
    L.orbfe_stream_set_queue_slots.argtypes = [vp, ci]
    L.orbfe_stream_queue_slots.argtypes = [vp]
    L.orbfe_stream_push.argtypes = [vp, vp, ci, ci, ci, C.c_size_t]
    L.orbfe_stream_pop.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.orbfe_stream_pop_hold.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(ci)]
    L.orbfe_stream_release.argtypes = [vp, ci]
    L.orbfe_stream_set_isolated_batches.argtypes = [vp, ci]
    L.orbfe_stream_batches_in_flight.argtypes = [vp]
    L.orbfe_stream_multi_create.argtypes = [ci, cf, ci, ci, ci, C.POINTER(ci), ci, ci, ci, C.POINTER(vp)]
    L.orbfe_stream_multi_destroy.argtypes = [vp]
    L.orbfe_stream_multi_destroy.restype = None
    L.orbfe_stream_multi_devices.argtypes = [vp]
    L.orbfe_stream_multi_capacity.argtypes = [vp]
    L.orbfe_stream_multi_device_of_next_push.argtypes = [vp]
    L.orbfe_stream_multi_set_matching.argtypes = [vp, vp, ci, cf, ci]
    L.orbfe_stream_multi_set_blur_variant.argtypes = [vp, ci]
    L.orbfe_stream_multi_push.argtypes = [vp, vp, ci, ci, ci, C.c_size_t]
    L.orbfe_stream_multi_pop.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.orbfe_stream_stats.argtypes = [vp, vp, ci]
    L.orbfe_stream_kernel_ms.argtypes = [vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), ci]
    L.orbfe_debug_quadtree.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, ci, C.POINTER(ci)]
    L.orbfe_debug_sincos_host_check.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_longlong)]
    L.orbfe_debug_logf.argtypes = [vp, vp, ci, vp]
    L.orbfe_debug_logf_host_check.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_longlong)]
    L.orbfe_local_map_create.argtypes = [vp, ci, C.POINTER(vp)]
    L.orbfe_local_map_destroy.argtypes = [vp]
    L.orbfe_local_map_destroy.restype = None
    L.orbfe_local_map_capacity.argtypes = [vp]
    L.orbfe_local_map_set_rows.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_local_map_refresh_rows.argtypes = [vp, vp, ci, ci, vp, vp, vp, ci, ci] + [vp] * 11
    L.orbfe_local_map_download_rows.argtypes = [vp, ci, vp, vp]
    L.orbfe_covisibility_counts.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, C.POINTER(ci)]
    L.orbfe_debug_covis_slots_per_pass.argtypes = []
    L.orbfe_debug_covis_ms.argtypes = [vp, vp]
    L.orbfe_redundant_observations.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp]
    L.orbfe_debug_culling_ms.argtypes = [vp, vp]
    L.orbfe_project_local_map.argtypes = [vp, vp, vp, vp, cf, vp, vp, ci, vp, vp, vp, vp, C.POINTER(ci)]
    L.orbfe_search_local_points_frame.argtypes = [vp, vp, vp, vp, cf, vp, vp, ci, vp, ci, vp, cf, cf, vp, vp, vp, vp, vp,
                                                  C.POINTER(ci), C.POINTER(ci)]
    L.orbfe_project_sources.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, C.POINTER(ci)]
    L.orbfe_search_by_projection_sources_frame.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp, ci, vp, ci, vp, cf, ci, ci, vp, vp, vp,
                                                           vp, C.POINTER(ci), C.POINTER(ci)]
    L.orbfe_project_keyframe.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, cf, vp, vp, vp, vp, C.POINTER(ci)]
    L.orbfe_search_projected_keyframe_frame.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, cf, vp, ci, vp, C.c_double, ci, vp, vp,
                                                        vp, vp, vp, C.POINTER(ci), C.POINTER(ci)]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceRows:
    """Descriptor rows [n][32] in device memory (Frame.descriptors_device()); accepted wherever the searches on resident
    frames take query descriptor rows."""

    def __init__(self, ptr, n):
        self.ptr, self.n = int(ptr), int(n)

    def __len__(self):
        return self.n


def _rows(a):
    """(argument for the C call, object to keep alive) for query descriptor rows: numpy array or DeviceRows."""
    if isinstance(a, DeviceRows):
        return C.c_void_p(a.ptr), a
    a = np.ascontiguousarray(a, np.uint8)
    return _p(a), a


def _check(rc):
    if rc != 0:
        raise OrbfeError(rc, load_library().orbfe_last_error().decode('utf-8', 'replace'))


def device_count():
    return load_library().orbfe_device_count()


def hamming(a, b):
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    return load_library().orbfe_hamming(_p(a), _p(b))


class Extractor:
    """ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) on one GPU."""

    def __init__(self, nfeatures=1000, scale=1.2, nlevels=8, ini_th=20, min_th=7, device=0):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.orbfe_extractor_create(nfeatures, scale, nlevels, ini_th, min_th, device, C.byref(h)))
        self.h = h
        self.nlevels = nlevels
        self.cap = self.L.orbfe_extractor_max_keypoints(h)

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_extractor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tables(self):
        n = self.nlevels
        sf, isf, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        nf = np.zeros(n, np.int32)
        _check(self.L.orbfe_extractor_scale_tables(self.h, _p(sf), _p(isf), _p(s2), _p(is2)))
        _check(self.L.orbfe_extractor_features_per_level(self.h, _p(nf)))
        return dict(sf=sf, isf=isf, s2=s2, is2=is2, nfeat=nf)

    def __call__(self, image):
        """image: (H, W) uint8 host array -> (keypoints[KP_DTYPE], descriptors[n,32] uint8)."""
        image = np.asarray(image)
        if image.size == 0:
            n = C.c_int(0)
            _check(self.L.orbfe_extract(self.h, None, 0, 0, 0, None, None, 0, C.byref(n)))
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2 and image.strides[1] == 1
        cap = max(self.cap, self.L.orbfe_extractor_max_keypoints_for_size(self.h, image.shape[0], image.shape[1]))
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        _check(self.L.orbfe_extract(self.h, _p(image), image.shape[0], image.shape[1], image.strides[0], _p(kps),
                                    _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    FORMATS = {'gray': 0, 'rgb': 1, 'bgr': 2, 'rgba': 3, 'bgra': 4}

    def set_blur_variant(self, variant):
        """0 = ORBFE_GAUSS_ED (GaussianBlur of OpenCV >= 4.1.1, the default), 1 = ORBFE_GAUSS_ROUNDED (OpenCV 4.0.0 - 4.1.0)."""
        _check(self.L.orbfe_extractor_set_blur_variant(self.h, int(variant)))

    def set_input_format(self, fmt='gray', variant=0):
        """Frames of later calls are interleaved 8-bit `fmt` pixels; variant 0 = 15-bit, 1 = 14-bit coefficients."""
        _check(self.L.orbfe_extractor_set_input_format(self.h, self.FORMATS[fmt], variant))

    def set_camera(self, fx, fy, cx, cy, dist=(), mode=0):
        """Frame::UndistortKeyPoints on the GPU for later calls (mode 0 = pinhole with dist = k1 k2 p1 p2 [k3 [k4 k5 k6]]; mode 1, the
        equidistant model, raises OrbfeError with code -6)."""
        d = np.ascontiguousarray(dist, np.float32)
        _check(self.L.orbfe_extractor_set_camera(self.h, mode, fx, fy, cx, cy, _p(d) if len(d) else None, len(d)))

    def set_camera_equidistant(self, fx, fy, cx, cy):
        """os1's equidistant fisheye model on the GPU for later calls: certified rounding in the kernel, the few undecided points
        settled with the host's std::tan (orbfe_extractor_set_camera_equidistant)."""
        _check(self.L.orbfe_extractor_set_camera_equidistant(self.h, fx, fy, cx, cy))

    def undistort_verdict(self, xy):
        """The equidistant kernel's raw output on (n, 2) float32 points, nothing settled -> (xy, undecided flags)."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out, flags = np.zeros_like(xy), np.zeros(len(xy), np.uint8)
        _check(self.L.orbfe_extractor_undistort_verdict(self.h, _p(xy) if len(xy) else None, len(xy), _p(out) if len(xy) else None,
                                                        _p(flags) if len(xy) else None))
        return out, flags.astype(bool)

    def equidistant_stats(self):
        """[points settled on the host, points whose value changed, match rows redone] of this handle."""
        out = np.zeros(3, np.int64)
        _check(self.L.orbfe_extractor_equidistant_stats(self.h, _p(out)))
        return out

    def undistort(self, xy):
        """The undistortion kernel on (n, 2) float32 points, with the camera of set_camera / set_camera_equidistant."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2).copy()
        _check(self.L.orbfe_extractor_undistort(self.h, _p(xy) if len(xy) else None, len(xy)))
        return xy

    def extract_undistorted(self, image):
        """image -> (keypoints, descriptors, xy_un[n, 2]): mvKeys, mDescriptors and mvKeysUn of one frame."""
        image = np.asarray(image)
        assert image.dtype == np.uint8 and image.ndim == 2 and image.strides[1] == 1
        cap = max(self.cap, self.L.orbfe_extractor_max_keypoints_for_size(self.h, image.shape[0], image.shape[1]))
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        xy = np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        _check(self.L.orbfe_extract_undistorted(self.h, _p(image), image.shape[0], image.shape[1], image.strides[0], _p(kps),
                                                _p(desc), cap, C.byref(n), _p(xy)))
        return kps[:n.value].copy(), desc[:n.value].copy(), xy[:n.value].copy()

    def collect_undistorted(self, matched=False):
        """collect() plus xy_un[B, cap, 2]; matched=True (after submit_matched_ptrs): also (matches12[B, cap], nmatches[B])."""
        B = self._pendingB
        kps = np.zeros((B, self.cap), KP_DTYPE)
        desc = np.zeros((B, self.cap, 32), np.uint8)
        xy = np.zeros((B, self.cap, 2), np.float32)
        n = np.zeros(B, np.int32)
        m12 = np.full((B, self.cap), -1, np.int32) if matched else None
        nm = np.zeros(B, np.int32) if matched else None
        _check(self.L.orbfe_extract_batch_collect_undistorted(self.h, _p(kps), _p(desc), self.cap, _p(n), _p(xy),
                                                              _p(m12) if matched else None, _p(nm) if matched else None))
        return (kps, desc, n, xy, m12, nm) if matched else (kps, desc, n, xy)

    def match_chain(self):
        """A predecessor chain for submit_matched_ptrs (orbfe_sfi_chain_create); free it with free_match_chain."""
        c = C.c_void_p()
        _check(self.L.orbfe_sfi_chain_create(self.h, C.byref(c)))
        return c

    def free_match_chain(self, chain):
        self.L.orbfe_sfi_chain_destroy(chain)

    def submit_matched_ptrs(self, chain, ptrs, rows, cols, stride, on_device, bounds, window=100, nnratio=0.9, check_ori=True):
        """orbfe_extract_batch_submit_matched: the batch, with SearchForInitialization of every frame against its predecessor."""
        B = len(ptrs)
        self._pending = (C.c_void_p * B)(*ptrs)
        self._pendingB = B
        b = np.asarray(bounds, np.float32)
        _check(self.L.orbfe_extract_batch_submit_matched(self.h, chain, B, self._pending, int(on_device), rows, cols, stride, _p(b),
                                                         window, nnratio, int(check_ori)))

    def extract_color(self, image):
        """image: (H, W, 3|4) uint8 host array in the format given to set_input_format."""
        image = np.ascontiguousarray(image, np.uint8)
        kps = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n = C.c_int(0)
        _check(self.L.orbfe_extract(self.h, _p(image), image.shape[0], image.shape[1], image.strides[0], _p(kps),
                                    _p(desc), self.cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def set_vocabulary(self, voc, levelsup=4):
        """Fuse Frame::ComputeBoW behind the descriptor kernel (voc: api.Vocabulary or None)."""
        self._voc = voc                                  # keep it alive
        _check(self.L.orbfe_extractor_set_vocabulary(self.h, voc.h if voc is not None else None, levelsup))

    def bow(self, frame, n):
        """BoW of frame `frame` of the last collected batch (n = its keypoint count), layout of Vocabulary.transform."""
        ids = np.zeros(max(n, 1), np.uint32)
        vals = np.zeros(max(n, 1), np.float64)
        fvn = np.zeros(max(n, 1), np.uint32)
        fvo = np.zeros(n + 1, np.uint32)
        fvf = np.zeros(max(n, 1), np.uint32)
        wof = np.zeros(max(n, 1), np.uint32)
        nof = np.zeros(max(n, 1), np.uint32)
        nw, nn = C.c_int(0), C.c_int(0)
        _check(self.L.orbfe_extract_bow(self.h, frame, _p(ids), _p(vals), C.byref(nw), _p(fvn), _p(fvo), _p(fvf), C.byref(nn),
                                        _p(wof), _p(nof)))
        nw, nn = nw.value, nn.value
        return ids[:nw], vals[:nw], (fvn[:nn], fvo[:nn + 1], fvf[:int(fvo[nn])]), wof[:n], nof[:n]

    def extract_batch_ptrs(self, ptrs, rows, cols, stride, on_device, kps=None, desc=None):
        """ptrs: sequence of raw addresses (host or device).  Returns (kps[B,cap], desc[B,cap,32], n[B])."""
        B = len(ptrs)
        arr = (C.c_void_p * B)(*ptrs)
        if kps is None:
            kps = np.zeros((B, self.cap), KP_DTYPE)
        if desc is None:
            desc = np.zeros((B, self.cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        _check(self.L.orbfe_extract_batch(self.h, B, arr, int(on_device), rows, cols, stride, _p(kps), _p(desc),
                                          int(kps.shape[1]), _p(n)))   # cap = what the caller's buffers hold per frame
        return kps, desc, n

    def submit_ptrs(self, ptrs, rows, cols, stride, on_device):
        """Enqueue a batch (returns immediately); collect() waits for it."""
        B = len(ptrs)
        self._pending = (C.c_void_p * B)(*ptrs)          # keep the pointer array alive
        self._pendingB = B
        _check(self.L.orbfe_extract_batch_submit(self.h, B, self._pending, int(on_device), rows, cols, stride))

    def wait(self):
        """orbfe_extract_batch_wait: the GPU side of the submitted batch is done when this returns; collect() then only assembles."""
        _check(self.L.orbfe_extract_batch_wait(self.h))

    def collect(self, kps=None, desc=None):
        B = self._pendingB
        if kps is None:
            kps = np.zeros((B, self.cap), KP_DTYPE)
        if desc is None:
            desc = np.zeros((B, self.cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        _check(self.L.orbfe_extract_batch_collect(self.h, _p(kps), _p(desc), self.cap, _p(n)))
        return kps, desc, n

    def extract_batch(self, images):
        images = [np.ascontiguousarray(im, np.uint8) for im in images]
        rows, cols = images[0].shape
        assert all(im.shape == (rows, cols) for im in images)
        kps, desc, n = self.extract_batch_ptrs([im.ctypes.data for im in images], rows, cols, cols, False)
        return [(kps[i, :n[i]].copy(), desc[i, :n[i]].copy()) for i in range(len(images))]

    # ---- stage accessors (parity tests) -------------------------------------------------------
    def level(self, level, frame=0):
        w, h = C.c_int(), C.c_int()
        _check(self.L.orbfe_debug_level_size(self.h, level, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(self.L.orbfe_debug_level_copy(self.h, frame, level, _p(out)))
        return out

    def candidates(self, level, frame=0):
        n = C.c_int(0)
        _check(self.L.orbfe_debug_candidates(self.h, frame, level, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.int32)
        _check(self.L.orbfe_debug_candidates(self.h, frame, level, _p(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def stage_ms(self):
        out = np.zeros(5, np.float32)
        _check(self.L.orbfe_debug_stage_ms(self.h, _p(out)))
        return out

    def kernel_ms(self, reset=False):
        """(ms[4] = pyramid, fast, compaction, describe; batches; frames) accumulated GPU time from HIP events."""
        ms = np.zeros(5, np.float64)
        b, f = C.c_longlong(0), C.c_longlong(0)
        _check(self.L.orbfe_debug_kernel_ms(self.h, _p(ms), C.byref(b), C.byref(f), int(reset)))
        return ms, b.value, f.value

    def set_profiling(self, enable=True):
        _check(self.L.orbfe_debug_set_profiling(self.h, int(enable)))

    def sincos(self, angle_deg):
        a = np.ascontiguousarray(angle_deg, np.float32)
        c = np.zeros_like(a)
        s = np.zeros_like(a)
        _check(self.L.orbfe_debug_sincos(self.h, _p(a), a.size, _p(c), _p(s)))
        return c, s


ERR_STALE = -7      # ORBFE_ERR_STALE: a raw triangulation row does not cover the flags it is finished with


class TriangulationNeighbour(C.Structure):
    """OrbfeTriangulationNeighbour: one neighbour of Matcher.search_for_triangulation_frames_batch."""
    _fields_ = [('frame2', C.c_void_p), ('has_mp2', C.c_void_p), ('fv2_nodes', C.c_void_p), ('fv2_offsets', C.c_void_p),
                ('fv2_features', C.c_void_p), ('n_fv2', C.c_int), ('F12', C.c_float * 9), ('ex', C.c_float), ('ey', C.c_float),
                ('scale_factors2', C.c_void_p), ('level_sigma2_2', C.c_void_p), ('nlevels2', C.c_int)]


def triangulation_finish(raw_row, has_mp1_initial, has_mp1_now, check_ori, kps1, kps2, n2=None):
    """One neighbour's SearchForTriangulation result from its raw row (Matcher.search_for_triangulation_frames_batch), with the
    current keyframe's flags as they stand NOW: mask, then the orientation histogram, then the pairs -> (nmatches, pairs[n,2]).
    Host only.  Raises OrbfeError with code ERR_STALE when has_mp1_now clears a flag has_mp1_initial had set."""
    L = load_library()
    raw = np.ascontiguousarray(raw_row, np.int32)
    h0, h1 = np.ascontiguousarray(has_mp1_initial, np.uint8), np.ascontiguousarray(has_mp1_now, np.uint8)
    assert len(h0) == len(raw) == len(h1)
    k1 = None if kps1 is None else np.ascontiguousarray(kps1, KP_DTYPE)
    k2 = None if kps2 is None else np.ascontiguousarray(kps2, KP_DTYPE)
    n2 = len(k2) if n2 is None else int(n2)
    pairs = np.full((max(len(raw), 1), 2), -1, np.int32)
    nm = C.c_int(0)
    _check(L.orbfe_triangulation_finish(_p(raw), len(raw), _p(h0), _p(h1), int(check_ori), None if k1 is None else _p(k1),
                                        None if k2 is None else _p(k2), n2, _p(pairs), C.byref(nm)))
    return nm.value, pairs[:nm.value]


class Camera(C.Structure):
    """OrbfeCamera: the current Frame's mRcw (row-major), mtcw, mOw, fx, fy, cx, cy and mfLogScaleFactor."""
    _fields_ = [('Rcw', C.c_float * 9), ('tcw', C.c_float * 3), ('Ow', C.c_float * 3), ('fx', C.c_float), ('fy', C.c_float),
                ('cx', C.c_float), ('cy', C.c_float), ('logScaleFactor', C.c_float)]

    @classmethod
    def make(cls, Rcw, tcw, Ow, fx, fy, cx, cy, log_scale_factor):
        c = cls()
        c.Rcw[:] = [float(v) for v in np.asarray(Rcw, np.float32).ravel()]
        c.tcw[:] = [float(v) for v in np.asarray(tcw, np.float32).ravel()]
        c.Ow[:] = [float(v) for v in np.asarray(Ow, np.float32).ravel()]
        c.fx, c.fy, c.cx, c.cy = float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy))
        c.logScaleFactor = float(np.float32(log_scale_factor))
        return c


class KeyFrameProjection(C.Structure):
    """OrbfeKeyFrameProjection: one projection loop of SearchByProjection(KeyFrame*, Scw), Fuse, Fuse(Scw) or a direction of
    SearchBySim3 -- the matrices the caller computed once, the intrinsics, and the three switches that tell the loops apart."""
    _fields_ = [('R', C.c_float * 9), ('t', C.c_float * 3), ('has_second', C.c_int), ('sR', C.c_float * 9), ('t2', C.c_float * 3),
                ('Ow', C.c_float * 3), ('fx', C.c_float), ('fy', C.c_float), ('cx', C.c_float), ('cy', C.c_float),
                ('logScaleFactor', C.c_float), ('invz_in_double', C.c_int), ('check_viewing_angle', C.c_int),
                ('distance_from_camera_point', C.c_int)]

    @classmethod
    def make(cls, R, t, fx, fy, cx, cy, log_scale_factor, Ow=None, sR=None, t2=None, invz_in_double=False,
             check_viewing_angle=True, distance_from_camera_point=False):
        """sR, t2: the second transform (SearchBySim3); Ow may be None only with distance_from_camera_point"""
        c = cls()
        f = lambda a: [float(v) for v in np.asarray(a, np.float32).ravel()]
        c.R[:], c.t[:] = f(R), f(t)
        c.has_second = 0 if sR is None else 1
        if sR is not None:
            c.sR[:], c.t2[:] = f(sR), f(t2)
        if Ow is not None:
            c.Ow[:] = f(Ow)
        c.fx, c.fy, c.cx, c.cy = float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy))
        c.logScaleFactor = float(np.float32(log_scale_factor))
        c.invz_in_double = int(bool(invz_in_double))
        c.check_viewing_angle = int(bool(check_viewing_angle))
        c.distance_from_camera_point = int(bool(distance_from_camera_point))
        return c


MP_IN_VIEW, MP_BAD, MP_CANDIDATO, MP_OBSERVED, MP_SKIP = 1, 2, 4, 8, 16
OBS_KF_BAD = 1
REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH = 1, 2
SRC_LAST_FRAME, SRC_KEYFRAME = 0, 1


class LocalMap:
    """orbfe_local_map: `capacity` 64-byte MapPoint rows (pos, normal, raw mfMin/MaxDistance, descriptor) on the matcher's
    device, searched through that matcher."""

    def __init__(self, matcher, capacity):
        self.L = load_library()
        self.matcher = matcher
        h = C.c_void_p()
        _check(self.L.orbfe_local_map_create(matcher.h, capacity, C.byref(h)))
        self.h = h
        self.capacity = capacity

    def set_rows(self, rows, pos=None, normal=None, min_raw=None, max_raw=None, desc=None):
        """Rows rows[i] := entry i of each given array (None: that field keeps its value).  Asynchronous, ordered before
        the matcher's next search."""
        rows = np.ascontiguousarray(rows, np.int32)
        keep = []

        def arg(a, dt, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt).reshape(shape)
            keep.append(a)
            return _p(a)
        n = len(rows)
        _check(self.L.orbfe_local_map_set_rows(self.h, n, _p(rows), arg(pos, np.float32, (n, 3)), arg(normal, np.float32, (n, 3)),
                                               arg(min_raw, np.float32, (n,)), arg(max_raw, np.float32, (n,)),
                                               arg(desc, np.uint8, (n, 32))))

    def refresh_rows(self, what, kf_frames, kf_Ow, rows, obs_offsets, obs_kf, obs_kp, obs_flags=None, ref_kf=None, ref_kp=None,
                     scale_factors=None, nlevels=None, outputs=True):
        """orbfe_local_map_refresh_rows: MapPoint::ComputeDistinctiveDescriptors (REFRESH_DESCRIPTOR) and / or
        UpdateNormalAndDepth (REFRESH_NORMAL_DEPTH) for the MapPoints in rows `rows`, from the resident keyframes `kf_frames`
        (api.Frame or None per slot) into the table.  Observations of MapPoint p: entries obs_offsets[p]..obs_offsets[p+1] of
        obs_kf (slot), obs_kp (keypoint), obs_flags (OBS_KF_BAD).  outputs=True returns (best_obs, normal [n, 3], min_raw,
        max_raw) as the rows hold them after the call; outputs=False only enqueues the work and returns None."""
        rows = np.ascontiguousarray(rows, np.int32)
        n = len(rows)
        offs = np.ascontiguousarray(obs_offsets, np.int32)
        okf = np.ascontiguousarray(obs_kf, np.int32)
        okp = np.ascontiguousarray(obs_kp, np.int32)
        ofl = None if obs_flags is None else np.ascontiguousarray(obs_flags, np.uint8)
        rkf = None if ref_kf is None else np.ascontiguousarray(ref_kf, np.int32)
        rkp = None if ref_kp is None else np.ascontiguousarray(ref_kp, np.int32)
        sf = None if scale_factors is None else np.ascontiguousarray(scale_factors, np.float32)
        if nlevels is None:
            nlevels = 1 if sf is None else len(sf)
        Ow = np.ascontiguousarray(kf_Ow, np.float32).reshape(-1, 3)
        handles = (C.c_void_p * max(len(kf_frames), 1))(*[None if f is None else f.h for f in kf_frames])
        best = np.zeros(max(n, 1), np.int32)
        nrm = np.zeros((max(n, 1), 3), np.float32)
        mn, mx = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        outs = [_p(best), _p(nrm), _p(mn), _p(mx)] if outputs else [None] * 4

        def q(a):
            return None if a is None else _p(a)
        _check(self.L.orbfe_local_map_refresh_rows(self.matcher.h, self.h, int(what), len(kf_frames), C.cast(handles, C.c_void_p), _p(Ow),
                                                   q(sf), int(nlevels), n, _p(rows), _p(offs), _p(okf), _p(okp), q(ofl), q(rkf),
                                                   q(rkp), *outs))
        return (best[:n], nrm[:n], mn[:n], mx[:n]) if outputs else None

    def download_rows(self, rows):
        """Test / debug: the 64-byte rows `rows` of the table as a uint8 array [n, 64]."""
        rows = np.ascontiguousarray(rows, np.int32)
        out = np.zeros((max(len(rows), 1), 64), np.uint8)
        _check(self.L.orbfe_local_map_download_rows(self.h, len(rows), _p(rows), _p(out)))
        return out[:len(rows)]

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_local_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frame:
    """A Frame's features resident on the GPU (orbfe_frame): mvKeysUn, mDescriptors and the grid, built once.  Pass it
    as the `kps` argument of Matcher.search_by_projection / _uv / search_projected (desc and bounds are then ignored)."""

    def __init__(self, handle, n):
        self.L = load_library()
        self.h = handle
        self.n = n

    @classmethod
    def from_host(cls, matcher, kps_un, desc, bounds):
        L = load_library()
        kps_un = np.ascontiguousarray(kps_un, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        b = np.asarray(bounds, np.float32)
        h = C.c_void_p()
        _check(L.orbfe_frame_create(matcher.h, _p(kps_un), _p(desc), len(kps_un), _p(b), C.byref(h)))
        return cls(h, len(kps_un))

    @classmethod
    def from_extract(cls, extractor, frame_index, bounds, xy_un=None):
        """Frame `frame_index` of the extractor's last collected batch, taken where the kernels left it."""
        L = load_library()
        b = np.asarray(bounds, np.float32)
        xy = None if xy_un is None else np.ascontiguousarray(xy_un, np.float32)
        h = C.c_void_p()
        _check(L.orbfe_frame_create_from_extract(extractor.h, frame_index, _p(b), None if xy is None else _p(xy), C.byref(h)))
        return cls(h, L.orbfe_frame_size(h))

    def __len__(self):
        return self.n

    def descriptors_device(self):
        """The frame's descriptor rows in device memory, keypoint order (valid while the frame lives)."""
        return DeviceRows(self.L.orbfe_frame_descriptors_device(self.h) or 0, self.n)

    def download(self):
        """(kps [x, y, angle, octave filled], desc, grid_order, cell_start) as they lie on the device."""
        k = np.zeros(max(self.n, 1), KP_DTYPE)
        d = np.zeros((max(self.n, 1), 32), np.uint8)
        order = np.zeros(max(self.n, 1), np.int32)
        cs = np.zeros(64 * 48 + 1, np.int32)
        _check(self.L.orbfe_frame_download(self.h, _p(k), _p(d), _p(order), _p(cs)))
        return k[:self.n], d[:self.n], order[:int(cs[-1])], cs

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class InitScores:
    """What Matcher.score_init_hypotheses* return: scores_h / scores_f (currentScore per hypothesis), best_h / best_f (winning
    hypothesis or -1), score_h / score_f (SH, SF), inliers_h / inliers_f (the winner's vbMatchesInliers as bool arrays) and
    n_matches.  The fields of a model that was not given are None."""

    __slots__ = ('scores_h', 'scores_f', 'best_h', 'best_f', 'score_h', 'score_f', 'inliers_h', 'inliers_f', 'n_matches')


class _InitScoreCall:
    """Argument tail and outputs of one orbfe_score_init_hypotheses* call."""

    def __init__(self, sigma, H21, H12, F21, cap):
        mats = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, 9) for a in (H21, H12, F21)]
        ks = {len(a) for a in mats if a is not None}
        if len(ks) > 1:
            raise ValueError('H21, H12 and F21 must hold the same number of hypotheses')
        self.K = ks.pop() if ks else 0
        self.mats = mats
        self.has_h, self.has_f = mats[0] is not None or mats[1] is not None, mats[2] is not None
        K = max(self.K, 1)
        self.scores = np.zeros((2, K), np.float32)
        self.best = np.full(2, -1, np.int32)
        self.best_score = np.zeros(2, np.float32)
        self.inl = np.zeros((2, max(cap, 1)), np.uint8)
        opt = lambda a: None if a is None else _p(a)
        self.tail = [float(sigma), self.K, opt(mats[0]), opt(mats[1]), opt(mats[2]), _p(self.scores[0]), _p(self.scores[1]),
                     _p(self.best[0:]), _p(self.best[1:]), _p(self.best_score[0:]), _p(self.best_score[1:]), _p(self.inl[0]),
                     _p(self.inl[1])]

    def result(self, n):
        r = InitScores()
        r.n_matches = int(n)
        for i, (has, sfx) in enumerate(((self.has_h, 'h'), (self.has_f, 'f'))):
            setattr(r, 'scores_' + sfx, self.scores[i, :self.K].copy() if has else None)
            setattr(r, 'best_' + sfx, int(self.best[i]) if has else None)
            setattr(r, 'score_' + sfx, np.float32(self.best_score[i]) if has else None)
            setattr(r, 'inliers_' + sfx, self.inl[i, :n].astype(bool) if has else None)
        return r


class _RansacCall:
    """Layout and outputs of one orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses call."""

    def __init__(self, L, row, corr, seg_off, hyp_seg, n_hyp):
        self.corr = np.ascontiguousarray(corr, np.float32).reshape(-1, row)
        if seg_off is None:                      # one segment: all correspondences, all hypotheses
            seg_off = [0, len(self.corr)]
            hyp_seg = np.zeros(n_hyp, np.int32) if hyp_seg is None else hyp_seg
        self.seg_off = np.ascontiguousarray(seg_off, np.int32)
        self.hyp_seg = np.ascontiguousarray(hyp_seg, np.int32)
        if len(self.hyp_seg) != n_hyp:
            raise ValueError('hyp_seg has one entry per hypothesis')
        if len(self.seg_off) < 2 or self.seg_off[-1] > len(self.corr):
            raise ValueError('seg_off has n_seg + 1 entries and ends inside corr')
        self.n_seg, self.n_hyp = len(self.seg_off) - 1, n_hyp
        words = L.orbfe_ransac_mask_words(self.n_seg, _p(self.seg_off), n_hyp, _p(self.hyp_seg))
        self.counts = np.zeros(max(n_hyp, 1), np.int32)
        self.words = np.zeros(max(int(words), 1), np.uint64)

    def result(self):
        """(counts [n_hyp] int32, masks: per hypothesis a bool array over its segment's correspondences)"""
        n = np.diff(self.seg_off.astype(np.int64))[self.hyp_seg]
        w = (n + 63) // 64
        start = np.concatenate([[0], np.cumsum(w)])
        bits = np.unpackbits(self.words.view(np.uint8), bitorder='little')
        masks = [bits[64 * start[k]:64 * start[k] + n[k]].astype(bool) for k in range(self.n_hyp)]
        return self.counts[:self.n_hyp].copy(), masks


class Matcher:
    """Hot subset of ORBmatcher on one GPU."""

    def score_sim3_hypotheses(self, corr, cams, T12, T21, seg_off=None, hyp_seg=None):
        """Sim3Solver::CheckInliers for every hypothesis of every solver (segment) in one call.  corr: [N][12] = X3Dc1, X3Dc2,
        P1im1, P2im2, maxErr1, maxErr2; cams: [n_seg][8] = fx fy cx cy of mK1, of mK2; T12 / T21: [K][12] float32, the top three
        rows of the 4x4; seg_off [n_seg + 1] / hyp_seg [K] (default: one segment).  -> (counts, per-hypothesis bool masks)."""
        T12 = np.ascontiguousarray(T12, np.float32).reshape(-1, 12)
        T21 = np.ascontiguousarray(T21, np.float32).reshape(-1, 12)
        if len(T12) != len(T21):
            raise ValueError('T12 and T21 hold the same number of hypotheses')
        c = _RansacCall(self.L, 12, corr, seg_off, hyp_seg, len(T12))
        cams = np.ascontiguousarray(cams, np.float32).reshape(-1, 8)
        if len(cams) != c.n_seg:
            raise ValueError('cams has one row per segment')
        _check(self.L.orbfe_score_sim3_hypotheses(self.h, c.n_seg, _p(c.seg_off), _p(c.corr), _p(cams), c.n_hyp, _p(c.hyp_seg), _p(T12),
                                                  _p(T21), _p(c.counts), None, _p(c.words)))
        return c.result()

    def score_pnp_hypotheses(self, corr, cams, Rt, seg_off=None, hyp_seg=None):
        """PnPsolver::CheckInliers for every hypothesis of every solver (segment) in one call.  corr: [N][6] = P3Dw, P2D, maxErr;
        cams: [n_seg][4] = uc vc fu fv (float64); Rt: [K][12] float64 = mRi row-major, then mti.  -> (counts, per-hypothesis
        bool masks)."""
        Rt = np.ascontiguousarray(Rt, np.float64).reshape(-1, 12)
        c = _RansacCall(self.L, 6, corr, seg_off, hyp_seg, len(Rt))
        cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 4)
        if len(cams) != c.n_seg:
            raise ValueError('cams has one row per segment')
        _check(self.L.orbfe_score_pnp_hypotheses(self.h, c.n_seg, _p(c.seg_off), _p(c.corr), _p(cams), c.n_hyp, _p(c.hyp_seg), _p(Rt),
                                                 _p(c.counts), None, _p(c.words)))
        return c.result()

    def score_init_hypotheses(self, pts, sigma, H21=None, H12=None, F21=None):
        """Initializer::CheckHomography / CheckFundamental for every hypothesis and the selection of FindHomography /
        FindFundamental.  pts: [n][4] = u1 v1 u2 v2 in match order; H21, H12, F21: [K][3][3] or [K][9] float32."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        c = _InitScoreCall(sigma, H21, H12, F21, len(pts))
        _check(self.L.orbfe_score_init_hypotheses(self.h, _p(pts), len(pts), *c.tail))
        return c.result(len(pts))

    def score_init_hypotheses_kps(self, kps1_un, kps2_un, matches12, sigma, H21=None, H12=None, F21=None):
        """The same from mvKeysUn of both frames and vnMatches12 (len(kps1_un) entries, -1 = unmatched)."""
        kps1_un = np.ascontiguousarray(kps1_un, KP_DTYPE)
        kps2_un = np.ascontiguousarray(kps2_un, KP_DTYPE)
        m12 = np.ascontiguousarray(matches12, np.int32)
        if len(m12) != len(kps1_un):
            raise ValueError('matches12 has one entry per keypoint of frame 1')
        c = _InitScoreCall(sigma, H21, H12, F21, len(kps1_un))
        n = C.c_int(0)
        _check(self.L.orbfe_score_init_hypotheses_kps(self.h, _p(kps1_un), len(kps1_un), _p(kps2_un), len(kps2_un), _p(m12), *c.tail,
                                                      C.byref(n)))
        return c.result(n.value)

    def score_init_hypotheses_frames(self, frame1, frame2, matches12, sigma, H21=None, H12=None, F21=None):
        """The same with both frames resident (Frame): only matches12 and the hypotheses are uploaded."""
        m12 = np.ascontiguousarray(matches12, np.int32)
        if len(m12) != len(frame1):
            raise ValueError('matches12 has one entry per keypoint of frame 1')
        c = _InitScoreCall(sigma, H21, H12, F21, len(frame1))
        n = C.c_int(0)
        _check(self.L.orbfe_score_init_hypotheses_frames(self.h, frame1.h, frame2.h, _p(m12), *c.tail, C.byref(n)))
        return c.result(n.value)

    def frame(self, kps_un, desc, bounds):
        return Frame.from_host(self, kps_un, desc, bounds)

    def resolve_rounds(self):
        return int(self.L.orbfe_debug_resolve_rounds(self.h))

    def resolve_route(self):
        return int(self.L.orbfe_debug_resolve_route(self.h))

    def resolve_phases(self):
        """Shader-clock ticks spent in k_resolve's set-up, fixed point and output phases."""
        o = np.zeros(4, np.int32)
        _check(self.L.orbfe_debug_resolve_phases(self.h, _p(o)))
        return np.diff(o.astype(np.int64)) & 0xffffffff

    def __init__(self, device=0):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.orbfe_matcher_create(device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_matcher_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_for_initialization(self, kps1, desc1, kps2, desc2, bounds, prev_xy, window=100, nnratio=0.9,
                                  check_ori=True):
        kps1 = np.ascontiguousarray(kps1, KP_DTYPE)
        kps2 = np.ascontiguousarray(kps2, KP_DTYPE)
        desc1 = np.ascontiguousarray(desc1, np.uint8)
        desc2 = np.ascontiguousarray(desc2, np.uint8)
        b = np.asarray(bounds, np.float32)
        prev = np.ascontiguousarray(prev_xy, np.float32).copy()
        m12 = np.full(max(len(kps1), 1), -1, np.int32)
        n = C.c_int(0)
        _check(self.L.orbfe_search_for_initialization(self.h, _p(kps1), _p(desc1), len(kps1), _p(kps2), _p(desc2),
                                                      len(kps2), _p(b), _p(prev), _p(m12), window, nnratio,
                                                      int(check_ori), C.byref(n)))
        return n.value, m12[:len(kps1)], prev

    def search_for_initialization_batch(self, pairs, bounds, window=100, nnratio=0.9, check_ori=True):
        """pairs: list of (kps1, desc1, kps2, desc2, prev_xy) with C-contiguous arrays.  Returns
        [(nmatches, matches12, prev_xy_out)] per pair; one GPU submission for all pairs."""
        P = len(pairs)
        k1 = [np.ascontiguousarray(p[0], KP_DTYPE) for p in pairs]
        d1 = [np.ascontiguousarray(p[1], np.uint8) for p in pairs]
        k2 = [np.ascontiguousarray(p[2], KP_DTYPE) for p in pairs]
        d2 = [np.ascontiguousarray(p[3], np.uint8) for p in pairs]
        prev = [np.ascontiguousarray(p[4], np.float32).copy() for p in pairs]
        m12 = [np.full(max(len(k), 1), -1, np.int32) for k in k1]
        arr = lambda xs: (C.c_void_p * P)(*[x.ctypes.data for x in xs])
        n1 = np.array([len(k) for k in k1], np.int32)
        n2 = np.array([len(k) for k in k2], np.int32)
        b = np.asarray(bounds, np.float32)
        nm = np.zeros(max(P, 1), np.int32)
        _check(self.L.orbfe_search_for_initialization_batch(self.h, P, arr(k1), arr(d1), _p(n1), arr(k2), arr(d2),
                                                            _p(n2), _p(b), arr(prev), arr(m12), window, nnratio,
                                                            int(check_ori), _p(nm)))
        return [(int(nm[i]), m12[i][:len(k1[i])], prev[i]) for i in range(P)]

    def search_by_projection(self, kps, desc, bounds, scale_factors, kp_occupied, mp_xy, mp_level, mp_viewcos,
                             mp_flags, mp_desc, th, nnratio):
        if isinstance(kps, Frame):
            sf = np.ascontiguousarray(scale_factors, np.float32)
            occ = np.ascontiguousarray(kp_occupied, np.uint8)
            mp_xy = np.ascontiguousarray(mp_xy, np.float32)
            mp_level = np.ascontiguousarray(mp_level, np.int32)
            mp_viewcos = np.ascontiguousarray(mp_viewcos, np.float32)
            mp_flags = np.ascontiguousarray(mp_flags, np.uint8)
            mp_desc_p, _keep = _rows(mp_desc)
            assigned = np.full(max(len(kps), 1), -1, np.int32)
            n = C.c_int(0)
            _check(self.L.orbfe_search_by_projection_frame(self.h, kps.h, _p(sf), len(sf), _p(occ), _p(mp_xy), _p(mp_level),
                                                           _p(mp_viewcos), _p(mp_flags), mp_desc_p, len(mp_level), th,
                                                           nnratio, _p(assigned), C.byref(n)))
            return n.value, assigned[:len(kps)]
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        b = np.asarray(bounds, np.float32)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        occ = np.ascontiguousarray(kp_occupied, np.uint8)
        mp_xy = np.ascontiguousarray(mp_xy, np.float32)
        mp_level = np.ascontiguousarray(mp_level, np.int32)
        mp_viewcos = np.ascontiguousarray(mp_viewcos, np.float32)
        mp_flags = np.ascontiguousarray(mp_flags, np.uint8)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8)
        assigned = np.full(max(len(kps), 1), -1, np.int32)
        n = C.c_int(0)
        _check(self.L.orbfe_search_by_projection(self.h, _p(kps), _p(desc), len(kps), _p(b), _p(sf), len(sf), _p(occ),
                                                 _p(mp_xy), _p(mp_level), _p(mp_viewcos), _p(mp_flags), _p(mp_desc),
                                                 len(mp_level), th, nnratio, _p(assigned), C.byref(n)))
        return n.value, assigned[:len(kps)]

    def search_by_projection_rows(self, frame, scale_factors, kp_occupied, mp_xy, mp_level, mp_viewcos, mp_flags, table, rows,
                                  th, nnratio):
        """orbfe_search_by_projection_frame_rows: the MapPoints' descriptors are rows of a DescTable (device copy + page-locked
        mirror); rows[i] = row number, bit 31 set = read that row from the mirror."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        occ = np.ascontiguousarray(kp_occupied, np.uint8)
        mp_xy = np.ascontiguousarray(mp_xy, np.float32)
        mp_level = np.ascontiguousarray(mp_level, np.int32)
        mp_viewcos = np.ascontiguousarray(mp_viewcos, np.float32)
        mp_flags = np.ascontiguousarray(mp_flags, np.uint8)
        rows = np.ascontiguousarray(rows, np.int32)
        assigned = np.full(max(len(frame), 1), -1, np.int32)
        n = C.c_int(0)
        _check(self.L.orbfe_search_by_projection_frame_rows(self.h, frame.h, _p(sf), len(sf), _p(occ), _p(mp_xy), _p(mp_level),
                                                            _p(mp_viewcos), _p(mp_flags), C.c_void_p(table.dev), C.c_void_p(table.host.base),
                                                            _p(rows), table.cap, len(mp_level), th, nnratio, _p(assigned), C.byref(n)))
        return n.value, assigned[:len(frame)]

    def project_local_map(self, frame, lmap, cam, rows, flags, cos_limit=0.5):
        """Frame::isInFrustum(pMP, cos_limit) for MapPoint i = row rows[i] of `lmap` (flags: MP_BAD / MP_SKIP skip it):
        dict of in_view, proj_xy, level, view_cos arrays and n_in_view."""
        rows = np.ascontiguousarray(rows, np.int32)
        flags = np.ascontiguousarray(flags, np.uint8)
        n = len(rows)
        iv = np.zeros(max(n, 1), np.uint8)
        xy = np.zeros((max(n, 1), 2), np.float32)
        lv = np.zeros(max(n, 1), np.int32)
        vc = np.zeros(max(n, 1), np.float32)
        cnt = C.c_int(0)
        _check(self.L.orbfe_project_local_map(self.h, frame.h, lmap.h, C.byref(cam), cos_limit, _p(rows), _p(flags), n, _p(iv),
                                              _p(xy), _p(lv), _p(vc), C.byref(cnt)))
        return dict(in_view=iv[:n], proj_xy=xy[:n], level=lv[:n], view_cos=vc[:n], n_in_view=cnt.value)

    def search_local_points(self, frame, lmap, cam, rows, flags, kp_occupied, scale_factors, th, nnratio=0.8, cos_limit=0.5):
        """Projection + SearchByProjection(F, vpLocalMapPoints, th) in one submission: dict of nmatches, kp_assigned,
        n_in_view and the projection's in_view, proj_xy, level, view_cos."""
        rows = np.ascontiguousarray(rows, np.int32)
        flags = np.ascontiguousarray(flags, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        occ = np.ascontiguousarray(kp_occupied, np.uint8)
        n = len(rows)
        iv = np.zeros(max(n, 1), np.uint8)
        xy = np.zeros((max(n, 1), 2), np.float32)
        lv = np.zeros(max(n, 1), np.int32)
        vc = np.zeros(max(n, 1), np.float32)
        assigned = np.full(max(len(frame), 1), -1, np.int32)
        nm, cnt = C.c_int(0), C.c_int(0)
        _check(self.L.orbfe_search_local_points_frame(self.h, frame.h, lmap.h, C.byref(cam), cos_limit, _p(rows), _p(flags), n,
                                                      _p(sf), len(sf), _p(occ), th, nnratio, _p(iv), _p(xy), _p(lv), _p(vc),
                                                      _p(assigned), C.byref(nm), C.byref(cnt)))
        return dict(nmatches=nm.value, kp_assigned=assigned[:len(frame)], n_in_view=cnt.value, in_view=iv[:n], proj_xy=xy[:n],
                    level=lv[:n], view_cos=vc[:n])

    def project_sources(self, cur, src, lmap, cam, mode, rows, flags):
        """The projection loop of SearchByProjection(CurrentFrame, LastFrame, th) (mode SRC_LAST_FRAME) or (CurrentFrame, pKF,
        sAlreadyFound, th, ORBdist) (SRC_KEYFRAME): source i = keypoint i of the resident frame `src`, its MapPoint row rows[i]
        of `lmap` (flags: MP_SKIP / MP_BAD skip it): dict of valid, uv, level arrays and n_valid."""
        rows = np.ascontiguousarray(rows, np.int32)
        flags = np.ascontiguousarray(flags, np.uint8)
        n = len(rows)
        va = np.zeros(max(n, 1), np.uint8)
        uv = np.zeros((max(n, 1), 2), np.float32)
        lv = np.zeros(max(n, 1), np.int32)
        cnt = C.c_int(0)
        _check(self.L.orbfe_project_sources(self.h, cur.h, src.h, lmap.h, C.byref(cam), mode, _p(rows), _p(flags), n, _p(va),
                                            _p(uv), _p(lv), C.byref(cnt)))
        return dict(valid=va[:n], uv=uv[:n], level=lv[:n], n_valid=cnt.value)

    def search_by_projection_sources(self, cur, src, lmap, cam, mode, rows, flags, kp_occupied, scale_factors, th, max_dist=100,
                                     check_ori=True):
        """project_sources + the rest of that search in one submission: dict of nmatches, kp_assigned (source index, -1, or -2
        for a slot the rotation check cleared), n_valid and the projection's valid, uv, level."""
        rows = np.ascontiguousarray(rows, np.int32)
        flags = np.ascontiguousarray(flags, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        occ = np.ascontiguousarray(kp_occupied, np.uint8)
        n = len(rows)
        va = np.zeros(max(n, 1), np.uint8)
        uv = np.zeros((max(n, 1), 2), np.float32)
        lv = np.zeros(max(n, 1), np.int32)
        assigned = np.full(max(len(cur), 1), -1, np.int32)
        nm, cnt = C.c_int(0), C.c_int(0)
        _check(self.L.orbfe_search_by_projection_sources_frame(self.h, cur.h, src.h, lmap.h, C.byref(cam), mode, _p(rows), _p(flags),
                                                               n, _p(sf), len(sf), _p(occ), th, int(max_dist), 1 if check_ori else 0,
                                                               _p(va), _p(uv), _p(lv), _p(assigned), C.byref(nm), C.byref(cnt)))
        return dict(nmatches=nm.value, kp_assigned=assigned[:len(cur)], n_valid=cnt.value, valid=va[:n], uv=uv[:n], level=lv[:n])

    def project_keyframe(self, kf, lmap, proj, rows, flags, scale_factors, th):
        """The projection loop of SearchByProjection(KeyFrame*, Scw) / Fuse / Fuse(Scw) / one direction of SearchBySim3 that
        `proj` (a KeyFrameProjection) describes: MapPoint i = row rows[i] of `lmap` (flags: MP_SKIP / MP_BAD skip it) into the
        resident keyframe `kf`: dict of valid, uv, level, radius arrays and n_valid."""
        rows = np.ascontiguousarray(rows, np.int32)
        flags = np.ascontiguousarray(flags, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        n = len(rows)
        va = np.zeros(max(n, 1), np.uint8)
        uv = np.zeros((max(n, 1), 2), np.float32)
        lv = np.zeros(max(n, 1), np.int32)
        ra = np.zeros(max(n, 1), np.float32)
        cnt = C.c_int(0)
        _check(self.L.orbfe_project_keyframe(self.h, kf.h, lmap.h, C.byref(proj), _p(rows), _p(flags), n, _p(sf), len(sf), th, _p(va),
                                             _p(uv), _p(lv), _p(ra), C.byref(cnt)))
        return dict(valid=va[:n], uv=uv[:n], level=lv[:n], radius=ra[:n], n_valid=cnt.value)

    def search_projected_keyframe(self, kf, lmap, proj, rows, flags, scale_factors, th, kp_skip=None, claim=False, inv_sigma2=None,
                                  chi2=5.99, max_dist=50):
        """project_keyframe + the projected best-match loop (search_projected) in one submission: dict of nmatches, best_idx,
        best_dist, n_valid and the projection's valid, uv, level."""
        rows = np.ascontiguousarray(rows, np.int32)
        flags = np.ascontiguousarray(flags, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        skip = None if kp_skip is None else np.ascontiguousarray(kp_skip, np.uint8)
        inv = None if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32)
        if inv is not None and len(inv) != len(sf):
            raise ValueError('inv_sigma2 holds one value per level')
        n = len(rows)
        va = np.zeros(max(n, 1), np.uint8)
        uv = np.zeros((max(n, 1), 2), np.float32)
        lv = np.zeros(max(n, 1), np.int32)
        bi = np.full(max(n, 1), -1, np.int32)
        bd = np.full(max(n, 1), -1, np.int32)
        nm, cnt = C.c_int(0), C.c_int(0)
        _check(self.L.orbfe_search_projected_keyframe_frame(self.h, kf.h, lmap.h, C.byref(proj), _p(rows), _p(flags), n, _p(sf),
                                                            len(sf), th, None if skip is None else _p(skip), int(claim),
                                                            None if inv is None else _p(inv), chi2, int(max_dist), _p(va), _p(uv),
                                                            _p(lv), _p(bi), _p(bd), C.byref(nm), C.byref(cnt)))
        return dict(nmatches=nm.value, best_idx=bi[:n], best_dist=bd[:n], n_valid=cnt.value, valid=va[:n], uv=uv[:n], level=lv[:n])

    def logf(self, x):
        """The device restatement of glibc logf, evaluated on this matcher's GPU."""
        a = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(a)
        _check(self.L.orbfe_debug_logf(self.h, _p(a), a.size, _p(out)))
        return out

    def upload_async(self, dst_device, src_host_ptr, nbytes):
        _check(self.L.orbfe_matcher_upload_async(self.h, C.c_void_p(dst_device), C.c_void_p(src_host_ptr), nbytes))

    def synchronize(self):
        _check(self.L.orbfe_matcher_synchronize(self.h))

    def search_by_projection_uv(self, kps, desc, bounds, scale_factors, kp_occupied, src_uv, src_level, src_angle,
                                src_flags, src_valid, src_desc, th, max_dist, skip_any_occupied, check_ori):
        if isinstance(kps, Frame):
            sf = np.ascontiguousarray(scale_factors, np.float32)
            occ = np.ascontiguousarray(kp_occupied, np.uint8)
            src_uv = np.ascontiguousarray(src_uv, np.float32)
            src_level = np.ascontiguousarray(src_level, np.int32)
            src_angle = np.ascontiguousarray(src_angle, np.float32)
            src_flags = np.ascontiguousarray(src_flags, np.uint8)
            src_valid = np.ascontiguousarray(src_valid, np.uint8)
            src_desc_p, _keep = _rows(src_desc)
            assigned = np.full(max(len(kps), 1), -1, np.int32)
            n = C.c_int(0)
            _check(self.L.orbfe_search_by_projection_uv_frame(self.h, kps.h, _p(sf), len(sf), _p(occ), _p(src_uv), _p(src_level),
                                                              _p(src_angle), _p(src_flags), _p(src_valid), src_desc_p,
                                                              len(src_level), th, max_dist, int(skip_any_occupied),
                                                              int(check_ori), _p(assigned), C.byref(n)))
            return n.value, assigned[:len(kps)]
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        b = np.asarray(bounds, np.float32)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        occ = np.ascontiguousarray(kp_occupied, np.uint8)
        src_uv = np.ascontiguousarray(src_uv, np.float32)
        src_level = np.ascontiguousarray(src_level, np.int32)
        src_angle = np.ascontiguousarray(src_angle, np.float32)
        src_flags = np.ascontiguousarray(src_flags, np.uint8)
        src_valid = np.ascontiguousarray(src_valid, np.uint8)
        src_desc = np.ascontiguousarray(src_desc, np.uint8)
        assigned = np.full(max(len(kps), 1), -1, np.int32)
        n = C.c_int(0)
        _check(self.L.orbfe_search_by_projection_uv(self.h, _p(kps), _p(desc), len(kps), _p(b), _p(sf), len(sf),
                                                    _p(occ), _p(src_uv), _p(src_level), _p(src_angle), _p(src_flags),
                                                    _p(src_valid), _p(src_desc), len(src_level), th, max_dist,
                                                    int(skip_any_occupied), int(check_ori), _p(assigned),
                                                    C.byref(n)))
        return n.value, assigned[:len(kps)]

    def window_candidates(self, kps, desc, bounds, qx, qy, qr, qmin, qmax, qdesc):
        """Ordered candidate lists (index, Hamming distance) per query -- the GPU part of every windowed search."""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        b = np.asarray(bounds, np.float32)
        qx, qy, qr = (np.ascontiguousarray(a, np.float32) for a in (qx, qy, qr))
        qmin, qmax = (np.ascontiguousarray(a, np.int32) for a in (qmin, qmax))
        qdesc = np.ascontiguousarray(qdesc, np.uint8)
        nq = len(qx)
        counts = np.zeros(max(nq, 1), np.uint32)
        offsets = np.zeros(max(nq, 1), np.uint32)
        cap = 1 << 16
        while True:
            pool = np.zeros(cap, np.uint32)
            used = C.c_size_t(0)
            rc = self.L.orbfe_window_candidates(self.h, _p(kps), _p(desc), len(kps), _p(b), nq, _p(qx), _p(qy), _p(qr),
                                                _p(qmin), _p(qmax), _p(qdesc), _p(counts), _p(offsets), _p(pool), cap,
                                                C.byref(used))
            if rc == -5:
                cap = int(used.value)
                continue
            _check(rc)
            break
        return [(pool[offsets[q]:offsets[q] + counts[q]] & 0xffff, pool[offsets[q]:offsets[q] + counts[q]] >> 16)
                for q in range(nq)]

    def distinctive_descriptors(self, desc_lists):
        """Batched MapPoint::ComputeDistinctiveDescriptors: list of (N_i, 32) arrays -> best index per list."""
        offs = np.zeros(len(desc_lists) + 1, np.int32)
        offs[1:] = np.cumsum([len(d) for d in desc_lists])
        allv = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in desc_lists])
                                     if len(desc_lists) and offs[-1] else np.zeros((1, 32), np.uint8))
        out = np.zeros(max(len(desc_lists), 1), np.int32)
        _check(self.L.orbfe_distinctive_descriptors(self.h, len(desc_lists), _p(offs), _p(allv), _p(out)))
        return out[:len(desc_lists)]

    def search_projected(self, kps, desc, bounds, uv, radius, level, valid, sdesc, kp_skip=None, claim=False,
                         inv_sigma2=None, chi2=5.99, max_dist=50):
        """Projected best-match loop of SearchByProjection(KF, Scw) / Fuse / SearchBySim3 -> (n, best_idx, best_dist)."""
        if isinstance(kps, Frame):
            uv = np.ascontiguousarray(uv, np.float32)
            radius = np.ascontiguousarray(radius, np.float32)
            level = np.ascontiguousarray(level, np.int32)
            valid = np.ascontiguousarray(valid, np.uint8)
            sdesc_p, _keep = _rows(sdesc)
            ns = len(radius)
            skip = None if kp_skip is None else np.ascontiguousarray(kp_skip, np.uint8)
            inv = None if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32)
            bi = np.full(max(ns, 1), -1, np.int32)
            bd = np.full(max(ns, 1), -1, np.int32)
            nm = C.c_int(0)
            _check(self.L.orbfe_search_projected_frame(self.h, kps.h, ns, _p(uv), _p(radius), _p(level), _p(valid), sdesc_p,
                                                       None if skip is None else _p(skip), int(claim),
                                                       None if inv is None else _p(inv), 0 if inv is None else len(inv), chi2,
                                                       max_dist, _p(bi), _p(bd), C.byref(nm)))
            return nm.value, bi[:ns], bd[:ns]
        kps = np.ascontiguousarray(kps)
        desc = np.ascontiguousarray(desc, np.uint8)
        b = np.asarray(bounds, np.float32)
        uv = np.ascontiguousarray(uv, np.float32)
        radius = np.ascontiguousarray(radius, np.float32)
        level = np.ascontiguousarray(level, np.int32)
        valid = np.ascontiguousarray(valid, np.uint8)
        sdesc = np.ascontiguousarray(sdesc, np.uint8)
        ns = len(radius)
        skip = None if kp_skip is None else np.ascontiguousarray(kp_skip, np.uint8)
        inv = None if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32)
        bi = np.full(max(ns, 1), -1, np.int32)
        bd = np.full(max(ns, 1), -1, np.int32)
        nm = C.c_int(0)
        _check(self.L.orbfe_search_projected(self.h, _p(kps), _p(desc), len(kps), _p(b), ns, _p(uv), _p(radius), _p(level),
                                             _p(valid), _p(sdesc), None if skip is None else _p(skip), int(claim),
                                             None if inv is None else _p(inv), 0 if inv is None else len(inv), chi2,
                                             max_dist, _p(bi), _p(bd), C.byref(nm)))
        return nm.value, bi[:ns], bd[:ns]

    def search_for_triangulation(self, kps1, desc1, has_mp1, fv1, kps2, desc2, has_mp2, fv2, F12, ex, ey, scale2, sigma2,
                                 check_ori=True):
        """ORBmatcher::SearchForTriangulation from the epipole onwards -> (nmatches, pairs[n,2])."""
        kps1 = np.ascontiguousarray(kps1)
        kps2 = np.ascontiguousarray(kps2)
        desc1 = np.ascontiguousarray(desc1, np.uint8)
        desc2 = np.ascontiguousarray(desc2, np.uint8)
        h1 = np.ascontiguousarray(has_mp1, np.uint8)
        h2 = np.ascontiguousarray(has_mp2, np.uint8)
        f1 = [np.ascontiguousarray(a, np.uint32) for a in fv1]
        f2 = [np.ascontiguousarray(a, np.uint32) for a in fv2]
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sc = np.ascontiguousarray(scale2, np.float32)
        sg = np.ascontiguousarray(sigma2, np.float32)
        pairs = np.full((max(len(kps1), 1), 2), -1, np.int32)
        nm = C.c_int(0)
        _check(self.L.orbfe_search_for_triangulation(self.h, _p(kps1), _p(desc1), _p(h1), len(kps1), _p(f1[0]), _p(f1[1]),
                                                     _p(f1[2]), len(f1[0]), _p(kps2), _p(desc2), _p(h2), len(kps2),
                                                     _p(f2[0]), _p(f2[1]), _p(f2[2]), len(f2[0]), _p(F), ex, ey, _p(sc),
                                                     _p(sg), len(sc), int(check_ori), _p(pairs), C.byref(nm)))
        return nm.value, pairs[:nm.value]

    @staticmethod
    def _tri_neighbours(neighbours):
        """(ctypes array of OrbfeTriangulationNeighbour, the arrays it points into) from [(frame2, has_mp2, fv2, F12, ex, ey,
        scale2, sigma2)]."""
        arr = (TriangulationNeighbour * max(len(neighbours), 1))()
        keep = []
        for t, (frame2, has2, fv2, F12, ex, ey, scale2, sigma2) in zip(arr, neighbours):
            h2 = np.ascontiguousarray(has2, np.uint8)
            f2 = [np.ascontiguousarray(a, np.uint32) for a in fv2]
            sc, sg = np.ascontiguousarray(scale2, np.float32), np.ascontiguousarray(sigma2, np.float32)
            keep += [frame2, h2, f2, sc, sg]
            t.frame2, t.has_mp2 = frame2.h, h2.ctypes.data
            t.fv2_nodes, t.fv2_offsets, t.fv2_features, t.n_fv2 = f2[0].ctypes.data, f2[1].ctypes.data, f2[2].ctypes.data, len(f2[0])
            t.F12 = (C.c_float * 9)(*[float(v) for v in np.asarray(F12, np.float32).reshape(9)])
            t.ex, t.ey = float(ex), float(ey)
            t.scale_factors2, t.level_sigma2_2, t.nlevels2 = sc.ctypes.data, sg.ctypes.data, len(sc)
        return arr, keep

    def search_for_triangulation_frames_batch(self, frame1, has_mp1, fv1, neighbours):
        """The SearchForTriangulation loop of LocalMapping::CreateNewMapPoints on resident keyframes in ONE GPU submission:
        frame1 (a Frame) against neighbours = [(frame2, has_mp2, fv2, F12, ex, ey, scale2, sigma2)].  Returns the raw rows
        [len(neighbours), len(frame1)] int32: the neighbour's keypoint for idx1, or -1 (nothing matched, or has_mp1 set); finish
        each row with triangulation_finish when the loop reaches its neighbour."""
        h1 = np.ascontiguousarray(has_mp1, np.uint8)
        f1 = [np.ascontiguousarray(a, np.uint32) for a in fv1]
        arr, _keep = self._tri_neighbours(neighbours)
        raw = np.full((len(neighbours), max(len(frame1), 1)), -1, np.int32)
        _check(self.L.orbfe_search_for_triangulation_frames_batch(self.h, frame1.h, _p(h1), _p(f1[0]), _p(f1[1]), _p(f1[2]), len(f1[0]),
                                                                  len(neighbours), C.cast(arr, C.c_void_p), _p(raw)))
        return raw[:, :len(frame1)]

    def search_for_triangulation_frames(self, frame1, has_mp1, fv1, neighbour, kps1=None, kps2=None, check_ori=True):
        """ORBmatcher::SearchForTriangulation on two resident keyframes (a batch of one, finished with the same flags)
        -> (nmatches, pairs[n,2]).  kps1 / kps2 (mvKeysUn, for their angles) are needed with check_ori."""
        h1 = np.ascontiguousarray(has_mp1, np.uint8)
        f1 = [np.ascontiguousarray(a, np.uint32) for a in fv1]
        arr, _keep = self._tri_neighbours([neighbour])
        k1 = None if kps1 is None else np.ascontiguousarray(kps1, KP_DTYPE)
        k2 = None if kps2 is None else np.ascontiguousarray(kps2, KP_DTYPE)
        pairs = np.full((max(len(frame1), 1), 2), -1, np.int32)
        nm = C.c_int(0)
        _check(self.L.orbfe_search_for_triangulation_frames(self.h, frame1.h, _p(h1), _p(f1[0]), _p(f1[1]), _p(f1[2]), len(f1[0]),
                                                            C.cast(arr, C.c_void_p), int(check_ori), None if k1 is None else _p(k1),
                                                            None if k2 is None else _p(k2), _p(pairs), C.byref(nm)))
        return nm.value, pairs[:nm.value]

    def search_by_bow(self, desc1, angle1, valid1, fv1, desc2, angle2, valid2, fv2, nnratio=0.7, check_ori=True,
                      strict=False):
        """ORBmatcher::SearchByBoW; fvX = (nodes, offsets, features) as returned by Vocabulary.transform.
        valid2=None is the (KeyFrame, Frame) overload, strict=True + valid2 the (KeyFrame, KeyFrame) one.
        Returns (nmatches, matches12)."""
        n1, n2 = len(desc1), len(desc2)                       # (numpy rows or DeviceRows: a resident frame's descriptors)
        d1p, _k1 = _rows(desc1)
        d2p, _k2 = _rows(desc2)
        angle1 = np.ascontiguousarray(angle1, np.float32)
        angle2 = np.ascontiguousarray(angle2, np.float32)
        valid1 = np.ascontiguousarray(valid1, np.uint8)
        v2 = None if valid2 is None else np.ascontiguousarray(valid2, np.uint8)
        f1 = [np.ascontiguousarray(a, np.uint32) for a in fv1]
        f2 = [np.ascontiguousarray(a, np.uint32) for a in fv2]
        m12 = np.full(max(n1, 1), -1, np.int32)
        nm = C.c_int(0)
        _check(self.L.orbfe_search_by_bow(self.h, d1p, _p(angle1), _p(valid1), n1, _p(f1[0]), _p(f1[1]),
                                          _p(f1[2]), len(f1[0]), d2p, _p(angle2), None if v2 is None else _p(v2),
                                          n2, _p(f2[0]), _p(f2[1]), _p(f2[2]), len(f2[0]), nnratio,
                                          int(check_ori), int(strict), _p(m12), C.byref(nm)))
        return nm.value, m12[:n1]

    def search_by_bow_batch(self, sides1, desc2, angle2, valid2, fv2, nnratio=0.7, check_ori=True, strict=False):
        """Tracking::Relocalization's SearchByBoW loop in one GPU submission: sides1 = [(desc1, angle1, valid1, fv1)] per
        candidate keyframe, all against one frame (side 2).  Returns [(nmatches, matches12)] per keyframe."""
        K = len(sides1)
        d1 = [np.ascontiguousarray(s[0], np.uint8) for s in sides1]
        a1 = [np.ascontiguousarray(s[1], np.float32) for s in sides1]
        v1 = [np.ascontiguousarray(s[2], np.uint8) for s in sides1]
        f1 = [[np.ascontiguousarray(a, np.uint32) for a in s[3]] for s in sides1]
        desc2 = np.ascontiguousarray(desc2, np.uint8)
        angle2 = np.ascontiguousarray(angle2, np.float32)
        v2 = None if valid2 is None else np.ascontiguousarray(valid2, np.uint8)
        f2 = [np.ascontiguousarray(a, np.uint32) for a in fv2]
        m12 = [np.full(max(len(d), 1), -1, np.int32) for d in d1]
        arr = lambda xs: (C.c_void_p * max(K, 1))(*[x.ctypes.data for x in xs])
        n1 = np.array([len(d) for d in d1] or [0], np.int32)
        nf1 = np.array([len(f[0]) for f in f1] or [0], np.int32)
        nm = np.zeros(max(K, 1), np.int32)
        _check(self.L.orbfe_search_by_bow_batch(self.h, K, arr(d1), arr(a1), arr(v1), _p(n1), arr([f[0] for f in f1]),
                                                arr([f[1] for f in f1]), arr([f[2] for f in f1]), _p(nf1), _p(desc2), _p(angle2),
                                                None if v2 is None else _p(v2), len(desc2), _p(f2[0]), _p(f2[1]), _p(f2[2]), len(f2[0]),
                                                nnratio, int(check_ori), int(strict), arr(m12), _p(nm)))
        return [(int(nm[k]), m12[k][:len(d1[k])]) for k in range(K)]

    def stage_ms(self):
        out = np.zeros(3, np.float64)
        _check(self.L.orbfe_debug_matcher_ms(self.h, _p(out)))
        return out

    def covis_ms(self):
        """The last covisibility_counts call, ms: host check + staging, kernel, whole call."""
        return self._three_ms(self.L.orbfe_debug_covis_ms)

    def redundant_observations(self, n_kf, obs_offsets, obs_kf, obs_level, subj_self, subj_offsets, subj_mp, subj_level, th_obs=3, mp_nobs=None):
        """The counts of LocalMapping::KeyFrameCulling for a batch of subjects: (n_mps, n_redundant); see redundant_observations."""
        return redundant_observations(self, n_kf, obs_offsets, obs_kf, obs_level, subj_self, subj_offsets, subj_mp, subj_level, th_obs, mp_nobs)

    def culling_ms(self):
        """The last redundant_observations call, ms: host check + staging, kernel, whole call."""
        return self._three_ms(self.L.orbfe_debug_culling_ms)

    def _three_ms(self, call):
        out = np.zeros(3, np.float64)
        _check(call(self.h, _p(out)))
        return out

    def get_features_in_area(self, kps, bounds, x, y, r, min_level, max_level):
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        b = np.asarray(bounds, np.float32)
        out = np.zeros(max(len(kps), 1), np.int32)
        n = C.c_int(0)
        _check(self.L.orbfe_debug_features_in_area(self.h, _p(kps), len(kps), _p(b), x, y, r, min_level, max_level,
                                                   _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()


def quadtree(x, y, score, min_x, max_x, min_y, max_y, n_target):
    """Product host quadtree (no GPU needed): indices of the retained candidates, list order."""
    x = np.ascontiguousarray(x, np.int16)
    y = np.ascontiguousarray(y, np.int16)
    score = np.ascontiguousarray(score, np.uint8)
    out = np.zeros(max(len(x), 1), np.int32)
    n = C.c_int(0)
    _check(load_library().orbfe_debug_quadtree(_p(x), _p(y), _p(score), len(x), min_x, max_x, min_y, max_y, n_target,
                                               _p(out), len(out), C.byref(n)))
    return out[:n.value].copy()


def undistort_equidistant(xy, fx, fy, cx, cy):
    """Frame::antidistorsionarProyeccionEquidistante (host helper of the C ABI)."""
    xy = np.ascontiguousarray(xy, np.float32).copy()
    _check(load_library().orbfe_undistort_equidistant(_p(xy), len(xy), fx, fy, cx, cy))
    return xy


def undistort_pinhole(xy, fx, fy, cx, cy, dist):
    """cv::undistortPoints(pts, pts, K, dist, Mat(), K) as Frame::UndistortKeyPoints calls it (host helper of the C ABI)."""
    xy = np.ascontiguousarray(xy, np.float32).copy()
    d = np.ascontiguousarray(dist, np.float32)
    _check(load_library().orbfe_undistort_pinhole(_p(xy), len(xy), fx, fy, cx, cy, _p(d) if len(d) else None, len(d)))
    return xy


def compute_image_bounds(cols, rows, mode, fx, fy, cx, cy, dist=()):
    """Frame::ComputeImageBounds -> (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    d = np.ascontiguousarray(dist, np.float32)
    b = np.zeros(4, np.float32)
    _check(load_library().orbfe_compute_image_bounds(cols, rows, mode, fx, fy, cx, cy, _p(d) if len(d) else None, len(d), _p(b)))
    return b


def sincos_host_mismatches(lo_bits, hi_bits, step=1):
    bad = C.c_longlong(0)
    _check(load_library().orbfe_debug_sincos_host_check(lo_bits, hi_bits, step, C.byref(bad)))
    return bad.value


def logf_host_mismatches(lo_bits, hi_bits, step=1):
    """Floats with bit patterns lo_bits, lo_bits + step, ... <= hi_bits on which the host build of the device logf
    restatement differs from the host libm."""
    bad = C.c_longlong(0)
    _check(load_library().orbfe_debug_logf_host_check(lo_bits, hi_bits, step, C.byref(bad)))
    return bad.value


def covis_slots_per_pass():
    """Observer slots one pass of k_covisibility counts (the bins of its LDS histogram)."""
    return load_library().orbfe_debug_covis_slots_per_pass()


def covisibility_bound(n_kf, obs_offsets, subj_offsets, subj_mp, subj_limit=None):
    """Sum over the subjects of min(limit, observations reachable from the subject): no covisibility_counts call needs more
    output entries.  (Entries outside [0, n_mp) count as skipped here; the library refuses them.)"""
    oo = np.asarray(obs_offsets, np.int64)
    so = np.asarray(subj_offsets, np.int64)
    mp = np.asarray(subj_mp, np.int64)
    n_subj = len(so) - 1
    if n_subj <= 0:
        return 0
    per_mp = np.diff(oo)
    ok = (mp >= 0) & (mp < len(per_mp))
    per_entry = np.zeros(len(mp) + 1, np.int64)
    per_entry[1:][ok] = np.maximum(per_mp[mp[ok]], 0)
    run = np.cumsum(per_entry)
    at = np.clip(so, 0, len(mp))
    reach = np.maximum(run[at[1:]] - run[at[:-1]], 0)
    limit = np.full(n_subj, n_kf, np.int64) if subj_limit is None else np.clip(np.asarray(subj_limit, np.int64), 0, max(n_kf, 0))
    return int(np.minimum(reach, limit).sum())


def _obs_graph(obs_offsets, obs_kf, subj_self, subj_offsets, subj_mp):
    """The observation graph covisibility_counts and redundant_observations both take: the five arrays as contiguous int32, n_mp,
    n_subj, and whether the two offset arrays have the lengths that go with them."""
    oo, ok, ss, so, sm = (np.ascontiguousarray(a, np.int32) for a in (obs_offsets, obs_kf, subj_self, subj_offsets, subj_mp))
    n_mp, n_subj = len(oo) - 1, len(ss)
    return (oo, ok, ss, so, sm), n_mp, n_subj, len(so) == n_subj + 1 and n_mp >= 0


def _pn(a):
    """the array's pointer, None for an empty or absent one (the C calls take a null payload with an empty CSR)"""
    return None if a is None or len(a) == 0 else _p(a)


def covisibility_counts(matcher, n_kf, obs_offsets, obs_kf, subj_self, subj_offsets, subj_mp, subj_limit=None, cap=None):
    """The counters of KeyFrame::UpdateConnections / Tracking::UpdateLocalKeyFrames for a batch of subjects
    (orbfe_covisibility_counts): MapPoint p is observed by the keyframe slots obs_kf[obs_offsets[p]:obs_offsets[p+1]]; subject s
    names the MapPoints subj_mp[subj_offsets[s]:subj_offsets[s+1]] (-1: skipped), excludes its own slot subj_self[s] (-1: nobody)
    and every slot >= subj_limit[s] (None: no limit).  Returns (out_offsets, out_kf, out_count): subject s owns
    [out_offsets[s], out_offsets[s+1]) of the non-zero counters in ascending slot order.  cap (None: covisibility_bound, which
    always suffices) is the room for entries; a call that needs more raises OrbfeError with code -5 and .n_needed set.
    matcher None reaches the library's argument check only (every call is then refused, with the reason)."""
    (oo, ok, ss, so, sm), n_mp, n_subj, fits = _obs_graph(obs_offsets, obs_kf, subj_self, subj_offsets, subj_mp)
    sl = None if subj_limit is None else np.ascontiguousarray(subj_limit, np.int32)
    if not fits or (sl is not None and len(sl) != n_subj):
        raise ValueError('covisibility_counts: obs_offsets needs n_mp + 1 entries, subj_offsets n_subj + 1, subj_limit n_subj')
    if cap is None:
        cap = covisibility_bound(n_kf, oo, so, sm, sl)
    out_offsets = np.zeros(n_subj + 1, np.int32)
    out_kf = np.zeros(max(cap, 1), np.int32)
    out_count = np.zeros(max(cap, 1), np.int32)
    needed = C.c_int(0)
    rc = load_library().orbfe_covisibility_counts(None if matcher is None else matcher.h, n_kf, n_mp, _p(oo), _pn(ok), n_subj, _pn(ss),
                                                  None if sl is None else _p(sl), _p(so), _pn(sm), _p(out_offsets), _p(out_kf), _p(out_count), cap,
                                                  C.byref(needed))
    if rc != 0:
        e = OrbfeError(rc, load_library().orbfe_last_error().decode('utf-8', 'replace'))
        e.n_needed = needed.value if rc == -5 else None
        raise e
    return out_offsets, out_kf[:needed.value].copy(), out_count[:needed.value].copy()


def redundant_observations(matcher, n_kf, obs_offsets, obs_kf, obs_level, subj_self, subj_offsets, subj_mp, subj_level, th_obs=3, mp_nobs=None):
    """The counting loop of LocalMapping::KeyFrameCulling for a batch of subjects (orbfe_redundant_observations).  The CSRs are
    those of covisibility_counts; obs_level / subj_level hold the octave (uint8) of every observation / entry, mp_nobs
    MapPoint::Observations() (None: the CSR's length per MapPoint).  Returns (n_mps, n_redundant), int32 per subject: the entries
    that name a MapPoint, and those of them whose MapPoint has more than th_obs observations of which at least th_obs are by other
    keyframes at a level <= the entry's + 1.  matcher None reaches the library's argument check only (every call is then
    refused, with the reason)."""
    (oo, ok, ss, so, sm), n_mp, n_subj, fits = _obs_graph(obs_offsets, obs_kf, subj_self, subj_offsets, subj_mp)
    ol = np.ascontiguousarray(obs_level, np.uint8)
    sv = np.ascontiguousarray(subj_level, np.uint8)
    nb = None if mp_nobs is None else np.ascontiguousarray(mp_nobs, np.int32)
    if not fits or len(ol) != len(ok) or len(sv) != len(sm) or (nb is not None and len(nb) != n_mp):
        raise ValueError('redundant_observations: obs_offsets needs n_mp + 1 entries, subj_offsets n_subj + 1, mp_nobs n_mp, a level per observation and entry')
    n_mps = np.zeros(max(n_subj, 1), np.int32)
    n_red = np.zeros(max(n_subj, 1), np.int32)
    L = load_library()
    rc = L.orbfe_redundant_observations(None if matcher is None else matcher.h, n_kf, n_mp, _p(oo), _pn(ok), _pn(ol),
                                        None if nb is None else _p(nb), n_subj, _pn(ss), _p(so), _pn(sm), _pn(sv), int(th_obs), _p(n_mps), _p(n_red))
    if rc != 0:
        raise OrbfeError(rc, L.orbfe_last_error().decode('utf-8', 'replace'))
    return n_mps[:n_subj].copy(), n_red[:n_subj].copy()


class Vocabulary:
    """DBoW2 ORB vocabulary resident in HBM; transform() = Frame::ComputeBoW."""

    def __init__(self, image, device=0):
        self.L = load_library()
        h = C.c_void_p()
        buf = np.frombuffer(image, np.uint8)
        _check(self.L.orbfe_vocabulary_create_from_image(device, _p(buf), buf.size, C.byref(h)))
        self.h = h

    def info(self):
        v = [C.c_int(0) for _ in range(6)]
        _check(self.L.orbfe_vocabulary_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(('k', 'L', 'scoring', 'weighting', 'n_nodes', 'n_words'), [x.value for x in v]))

    def assemble(self, leaf, node):
        """BowVector / FeatureVector from per-keypoint (leaf node, level node) pairs (Stream.bow_raw / orbfe_extract_bow_raw)."""
        leaf = np.ascontiguousarray(leaf, np.uint32)
        node = np.ascontiguousarray(node, np.uint32)
        n = len(leaf)
        ids = np.zeros(max(n, 1), np.uint32)
        vals = np.zeros(max(n, 1), np.float64)
        fvn = np.zeros(max(n, 1), np.uint32)
        fvo = np.zeros(n + 1, np.uint32)
        fvf = np.zeros(max(n, 1), np.uint32)
        wof = np.zeros(max(n, 1), np.uint32)
        nw, nn = C.c_int(0), C.c_int(0)
        _check(self.L.orbfe_bow_assemble(self.h, _p(leaf), _p(node), n, _p(ids), _p(vals), C.byref(nw), _p(fvn), _p(fvo), _p(fvf),
                                         C.byref(nn), _p(wof)))
        nw, nn = nw.value, nn.value
        return ids[:nw], vals[:nw], (fvn[:nn], fvo[:nn + 1], fvf[:int(fvo[nn])]), wof[:n], node[:n]

    def transform(self, desc, levelsup=4):
        """-> (bow_ids, bow_values, (fv_nodes, fv_offsets, fv_features), word_of_feature, node_of_feature)"""
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(desc)
        ids = np.zeros(max(n, 1), np.uint32)
        vals = np.zeros(max(n, 1), np.float64)
        fvn = np.zeros(max(n, 1), np.uint32)
        fvo = np.zeros(n + 1, np.uint32)
        fvf = np.zeros(max(n, 1), np.uint32)
        wof = np.zeros(max(n, 1), np.uint32)
        nof = np.zeros(max(n, 1), np.uint32)
        nw, nn = C.c_int(0), C.c_int(0)
        _check(self.L.orbfe_bow_transform(self.h, _p(desc), n, 0, levelsup, _p(ids), _p(vals), C.byref(nw), _p(fvn),
                                          _p(fvo), _p(fvf), C.byref(nn), _p(wof), _p(nof)))
        nw, nn = nw.value, nn.value
        return ids[:nw], vals[:nw], (fvn[:nn], fvo[:nn + 1], fvf[:int(fvo[nn])]), wof[:n], nof[:n]

    def transform_batch(self, descs, levelsup=4, capacity=None, out=None):
        """transform() of several descriptor sets in one submission (orbfe_bow_transform_batch) -> a list of transform()'s tuples.
        A set is an (n, 32) uint8 array (ordinary memory, or the view of a PinnedArray: read in place) or a DeviceRows (a resident
        frame's rows: read in place).  capacity: per-set output capacities (default: each set's size).  out: a BowBatchOutputs to
        write into instead of fresh arrays."""
        ns = len(descs)
        keep, ptr, n = [], np.zeros(max(ns, 1), np.uint64), np.zeros(max(ns, 1), np.int32)
        for s, d in enumerate(descs):
            if isinstance(d, DeviceRows):
                ptr[s], n[s] = d.ptr, d.n
            else:
                d = np.ascontiguousarray(d, np.uint8)
                keep.append(d)
                ptr[s], n[s] = (d.ctypes.data if len(d) else 0), len(d)
        cap = n.copy() if capacity is None else np.ascontiguousarray(capacity, np.int32)
        if out is None:
            out = BowBatchOutputs(cap[:ns])
        nw, nn = out.nw, out.nn
        tab = np.zeros((7, max(ns, 1)), np.uint64)
        for s in range(ns):
            for k in range(7):
                tab[k, s] = out[s][k].ctypes.data
        _check(self.L.orbfe_bow_transform_batch(self.h, levelsup, ns, _p(ptr), _p(n), _p(cap), _p(tab[0]), _p(tab[1]), _p(nw), _p(tab[2]),
                                                _p(tab[3]), _p(tab[4]), _p(nn), _p(tab[5]), _p(tab[6])))
        res = []
        for s in range(ns):
            ids, vals, fvn, fvo, fvf, wof, nof = out[s]
            a, b = int(nw[s]), int(nn[s])
            res.append((ids[:a], vals[:a], (fvn[:b], fvo[:b + 1], fvf[:int(fvo[b])]), wof[:int(n[s])], nof[:int(n[s])]))
        return res

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_vocabulary_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BowBatchOutputs(list):
    """Caller-owned outputs for Vocabulary.transform_batch(out=...): a list of per-set (ids, vals, fvn, fvo, fvf, wof, nof) arrays plus
    the n_words / n_fv_nodes arrays `nw` / `nn` -- for callers that want to see what a refused call left in them."""

    def __init__(self, capacities, fill=0):
        super().__init__()
        for c in capacities:
            c = int(c)
            t = (np.zeros(max(c, 1), np.uint32), np.zeros(max(c, 1), np.float64), np.zeros(max(c, 1), np.uint32),
                 np.zeros(max(c, 0) + 1, np.uint32), np.zeros(max(c, 1), np.uint32), np.zeros(max(c, 1), np.uint32),
                 np.zeros(max(c, 1), np.uint32))
            for a in t:
                a.view(np.uint8)[:] = fill
            self.append(t)
        self.nw = np.zeros(max(len(self), 1), np.int32)
        self.nn = np.zeros(max(len(self), 1), np.int32)
        self.nw.view(np.uint8)[:] = fill
        self.nn.view(np.uint8)[:] = fill


class KeyFrameDatabase:
    """The map's keyframe BowVectors resident in HBM (KeyFrameDatabase.cc's inverted file and mpVoc->score as one GPU query).
    scoring: the vocabulary's DBoW2 ScoringType (0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 5 DOT_PRODUCT; KL and BHATTACHARYYA raise)."""

    def __init__(self, n_words, scoring=0, capacity_keyframes=4096, capacity_entries=4096 * 1024, device=0):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.orbfe_kfdb_create(device, n_words, scoring, capacity_keyframes, capacity_entries, C.byref(h)))
        self.h = h
        self.capacity_keyframes = capacity_keyframes

    def add(self, key, words, values):
        """KeyFrameDatabase::add: `key` names the keyframe (any 64-bit integer not in the database), words ascending."""
        words = np.ascontiguousarray(words, np.uint32)
        values = np.ascontiguousarray(values, np.float64)
        assert words.shape == values.shape and words.ndim == 1
        _check(self.L.orbfe_kfdb_add(self.h, key, _p(words), _p(values), len(words)))

    def add_batch(self, keys, words, values):
        """add() for several keyframes in one call (orbfe_kfdb_add_batch): the database afterwards is the database after the single
        adds in order; an error at any entry raises and changes nothing."""
        n = len(keys)
        assert len(words) == n and len(values) == n
        keys = np.ascontiguousarray(keys, np.uint64)
        words = [np.ascontiguousarray(w, np.uint32) for w in words]
        values = [np.ascontiguousarray(v, np.float64) for v in values]
        pw = np.array([w.ctypes.data if len(w) else 0 for w in words] + [0], np.uint64)
        pv = np.array([v.ctypes.data if len(v) else 0 for v in values] + [0], np.uint64)
        cnt = np.array([len(w) for w in words] + [0], np.int32)
        assert all(w.shape == v.shape and w.ndim == 1 for w, v in zip(words, values))
        _check(self.L.orbfe_kfdb_add_batch(self.h, n, _p(keys) if n else None, _p(pw), _p(pv), _p(cnt)))

    def erase(self, key):
        _check(self.L.orbfe_kfdb_erase(self.h, key))

    def clear(self):
        _check(self.L.orbfe_kfdb_clear(self.h))

    def size(self):
        """-> (live keyframes, live (word, value) entries)"""
        nk, ne = C.c_int(0), C.c_int(0)
        _check(self.L.orbfe_kfdb_size(self.h, C.byref(nk), C.byref(ne)))
        return nk.value, ne.value

    def query(self, words, values):
        """-> (keys, common, scores): every keyframe sharing a word with the query, in the reference's lKFsSharingWords order."""
        words = np.ascontiguousarray(words, np.uint32)
        values = np.ascontiguousarray(values, np.float64)
        cap = max(self.size()[0], 1)
        keys = np.zeros(cap, np.uint64)
        common = np.zeros(cap, np.int32)
        scores = np.zeros(cap, np.float64)
        n = C.c_int(0)
        _check(self.L.orbfe_kfdb_query(self.h, _p(words), _p(values), len(words), _p(keys), _p(common), _p(scores), cap, C.byref(n)))
        return keys[:n.value], common[:n.value], scores[:n.value]

    def score(self, words, values, keys, out=None):
        """mpVoc->score(query, keyframe) for the given keys (LoopClosing.cc:125-140); an unknown key raises, `out` untouched."""
        words = np.ascontiguousarray(words, np.uint32)
        values = np.ascontiguousarray(values, np.float64)
        keys = np.ascontiguousarray(keys, np.uint64)
        scores = np.zeros(max(len(keys), 1), np.float64) if out is None else out
        _check(self.L.orbfe_kfdb_score(self.h, _p(words), _p(values), len(words), _p(keys), len(keys), _p(scores)))
        return scores[:len(keys)]

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_kfdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedArray:
    """A numpy array in page-locked HOST memory (orbfe_host_alloc): `.a` is the view.  Query descriptor rows kept in one
    are fetched by DMA straight from it by the `_frame` searches."""

    def __init__(self, shape, dtype=np.uint8):
        L = load_library()
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        p = C.c_void_p()
        _check(L.orbfe_host_alloc(max(n * dt.itemsize, 1), C.byref(p)))
        self.base = p.value
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(n * dt.itemsize, 1),))
        self.a = raw[:n * dt.itemsize].view(dt).reshape(shape)

    def free(self):
        if getattr(self, 'base', None):
            self.a = None
            load_library().orbfe_host_free(C.c_void_p(self.base))
            self.base = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DescTable:
    """A caller-maintained descriptor table for orbfe_search_by_projection_frame_rows: `cap` 32-byte rows in device memory
    (`dev`) and their page-locked host mirror (`host.a`, a numpy view)."""

    def __init__(self, cap, device=0):
        self.L = load_library()
        self.device, self.cap = device, cap
        self.host = PinnedArray((cap, 32), np.uint8)
        self.host.a[:] = 0
        p = C.c_void_p()
        _check(self.L.orbfe_device_malloc(device, cap * 32, C.byref(p)))
        self.dev = p.value

    def upload(self, matcher, lo, hi):
        """rows [lo, hi) of the mirror -> device, asynchronously on the matcher's stream"""
        matcher.upload_async(self.dev + lo * 32, self.host.base + lo * 32, (hi - lo) * 32)

    def free(self):
        if self.dev:
            self.L.orbfe_device_free(self.device, C.c_void_p(self.dev))
            self.dev = None
            self.host.free()


class RegisteredArray:
    """A numpy array the caller owns, page-locked and mapped for the GPU in place (orbfe_host_register); unregistered by close()."""

    def __init__(self, a):
        assert a.flags['C_CONTIGUOUS']
        self.L = load_library()
        self.a = a
        _check(self.L.orbfe_host_register(C.c_void_p(a.ctypes.data), a.nbytes))
        self.live = True

    def close(self):
        if self.live:
            self.L.orbfe_host_unregister(C.c_void_p(self.a.ctypes.data))
            self.live = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedFrames:
    """A stack of equally sized u8 frames in page-locked HOST memory (orbfe_host_alloc): the fast way to hand
    host frames to the extractor (in_device_memory == 0)."""

    def __init__(self, frames):
        L = load_library()
        self.rows, self.cols = frames[0].shape
        self.stride = self.cols
        self.n = len(frames)
        self.frame_bytes = self.rows * self.stride
        p = C.c_void_p()
        _check(L.orbfe_host_alloc(self.frame_bytes * self.n, C.byref(p)))
        self.base = p.value
        view = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self.n, self.rows, self.cols))
        for i, f in enumerate(frames):
            view[i] = f
        self.ptrs = [self.base + i * self.frame_bytes for i in range(self.n)]

    def free(self):
        if getattr(self, 'base', None):
            load_library().orbfe_host_free(C.c_void_p(self.base))
            self.base = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceFrames:
    """A stack of equally sized u8 frames resident in HBM (hipMalloc'd through the C ABI)."""

    def __init__(self, frames, device=0, stride=None):
        L = load_library()
        self.device = device
        self.rows, self.cols = frames[0].shape
        self.stride = stride or self.cols
        self.n = len(frames)
        self.frame_bytes = self.rows * self.stride
        p = C.c_void_p()
        _check(L.orbfe_device_malloc(device, self.frame_bytes * self.n, C.byref(p)))
        self.base = p.value
        for i, f in enumerate(frames):
            buf = np.zeros((self.rows, self.stride), np.uint8)
            buf[:, :self.cols] = f
            _check(L.orbfe_device_upload(device, C.c_void_p(self.base + i * self.frame_bytes), _p(buf), buf.size))
        self.ptrs = [self.base + i * self.frame_bytes for i in range(self.n)]

    def free(self):
        if getattr(self, 'base', None):
            load_library().orbfe_device_free(self.device, C.c_void_p(self.base))
            self.base = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_synchronize(device=0):
    _check(load_library().orbfe_device_synchronize(device))


def device_numa_node(device=0):
    return load_library().orbfe_device_numa_node(device)


def bind_thread_to_device(device=0):
    """Restrict the calling thread (and threads it creates later) to the CPUs of the GPU's NUMA node; 0 = unchanged."""
    return load_library().orbfe_bind_thread_to_device(device)


def h2d_rate_gbs(device, host_ptr, nbytes, reps=8):
    g = C.c_double(0)
    _check(load_library().orbfe_debug_h2d_rate(device, C.c_void_p(host_ptr), nbytes, reps, C.byref(g)))
    return g.value


def _result_views(B, cap, ptrs, copy):
    """(kps[B,cap], desc[B,cap,32], n[B], matches12[B,cap], nmatches[B]) over a runner's result pointers."""
    def view(ptr, dtype, shape):
        n = int(np.prod(shape))
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)
        return a.copy() if copy else a
    pk, pd, pn, pm, pnm = ptrs
    return (view(pk, KP_DTYPE, (B, cap)), view(pd, np.uint8, (B, cap, 32)), view(pn, np.int32, (B,)),
            view(pm, np.int32, (B, cap)), view(pnm, np.int32, (B,)))


class Stream:
    """Native stream runner (orbfe_stream_*): push batches of frames, pop (keypoints, descriptors, matches
    against the predecessor frame) in order.  Orchestration (async extraction, matching thread) is C++."""

    def __init__(self, nfeatures, scale, nlevels, ini_th, min_th, device, batch, depth=2):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.orbfe_stream_create(nfeatures, scale, nlevels, ini_th, min_th, device, batch, depth, C.byref(h)))
        self.h = h
        self.batch = batch
        self.cap = self.L.orbfe_stream_capacity(h)

    def set_queue_slots(self, nslots):
        """Result slots = batches that may be pushed ahead of the pops + 2 (default depth + 4)."""
        _check(self.L.orbfe_stream_set_queue_slots(self.h, int(nslots)))

    def queue_slots(self):
        return int(self.L.orbfe_stream_queue_slots(self.h))

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_matching(self, bounds, window=100, nnratio=0.9, check_ori=True):
        b = np.asarray(bounds, np.float32)
        _check(self.L.orbfe_stream_set_matching(self.h, _p(b), window, nnratio, int(check_ori)))

    def set_blur_variant(self, variant):
        _check(self.L.orbfe_stream_set_blur_variant(self.h, int(variant)))

    def set_vocabulary(self, voc, levelsup=4):
        self._voc = voc
        _check(self.L.orbfe_stream_set_vocabulary(self.h, voc.h if voc is not None else None, levelsup))

    def set_camera(self, fx, fy, cx, cy, dist=(), mode=0):
        """orbfe_stream_set_camera: streamed frames are matched on mvKeysUn; only while no batch is in flight."""
        d = np.ascontiguousarray(dist, np.float32)
        _check(self.L.orbfe_stream_set_camera(self.h, mode, fx, fy, cx, cy, _p(d) if len(d) else None, len(d)))

    def set_camera_equidistant(self, fx, fy, cx, cy):
        """orbfe_stream_set_camera_equidistant: the fisheye model, same rules as set_camera."""
        _check(self.L.orbfe_stream_set_camera_equidistant(self.h, fx, fy, cx, cy))

    def equidistant_stats(self):
        """[points settled on the host, points whose value changed, match rows redone], summed over the runner's handles."""
        out = np.zeros(3, np.int64)
        _check(self.L.orbfe_stream_equidistant_stats(self.h, _p(out)))
        return out

    def xy_un(self):
        """mvKeysUn [B, cap, 2] of the last popped batch (a copy)."""
        p = C.c_void_p()
        _check(self.L.orbfe_stream_xy_un(self.h, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(self.batch, self.cap, 2)).copy()

    def bow_raw(self, frame):
        """(leaf, node) arrays of frame `frame` of the last popped batch (copies)."""
        pl, pn, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        _check(self.L.orbfe_stream_bow_raw(self.h, frame, C.byref(pl), C.byref(pn), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        leaf = np.ctypeslib.as_array(C.cast(pl, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()
        node = np.ctypeslib.as_array(C.cast(pn, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()
        return leaf, node

    def push_ptrs(self, ptrs, rows, cols, stride, on_device=True):
        assert len(ptrs) == self.batch
        arr = (C.c_void_p * self.batch)(*ptrs)
        _check(self.L.orbfe_stream_push(self.h, arr, int(on_device), rows, cols, stride))
        self.cap = self.L.orbfe_stream_capacity(self.h)      # grows with a geometry that returns more keypoints

    def pop(self, copy=False):
        """-> (kps[B,cap], desc[B,cap,32], n[B], matches12[B,cap], nmatches[B]) as views valid until the next pop."""
        pk, pd, pn, pm, pnm = (C.c_void_p() for _ in range(5))
        _check(self.L.orbfe_stream_pop(self.h, C.byref(pk), C.byref(pd), C.byref(pn), C.byref(pm), C.byref(pnm)))
        return _result_views(self.batch, self.cap, (pk, pd, pn, pm, pnm), copy)

    def pop_hold(self, copy=False):
        """-> (ticket, (kps, desc, n, matches12, nmatches)): pop() whose views stay valid until release(ticket) (orbfe_stream_pop_hold)."""
        pk, pd, pn, pm, pnm = (C.c_void_p() for _ in range(5))
        t = C.c_int(-1)
        _check(self.L.orbfe_stream_pop_hold(self.h, C.byref(pk), C.byref(pd), C.byref(pn), C.byref(pm), C.byref(pnm), C.byref(t)))
        return t.value, _result_views(self.batch, self.cap, (pk, pd, pn, pm, pnm), copy)

    def release(self, ticket):
        """Give a held result's slot back to the runner (orbfe_stream_release)."""
        _check(self.L.orbfe_stream_release(self.h, int(ticket)))

    def batches_in_flight(self):
        """Batches the runner keeps on the GPU at a time: `depth`, or fewer when the process has fewer hardware queues than that."""
        return int(self.L.orbfe_stream_batches_in_flight(self.h))

    def set_isolated_batches(self, on=True):
        """Frame 0 of every batch has no predecessor (orbfe_stream_set_isolated_batches)."""
        _check(self.L.orbfe_stream_set_isolated_batches(self.h, int(on)))

    def stats(self, reset=False):
        """[submit ms, collect ms, match ms, batches done] since the last reset: the extract worker's busy time in submit and in
        collect (incl. waiting for the GPU).  Matching runs inside those calls, so the match slot is always 0."""
        out = np.zeros(4, np.float64)
        _check(self.L.orbfe_stream_stats(self.h, _p(out), int(reset)))
        return out

    def kernel_ms(self, reset=False):
        ms = np.zeros(5, np.float64)
        b, f = C.c_longlong(0), C.c_longlong(0)
        _check(self.L.orbfe_stream_kernel_ms(self.h, _p(ms), C.byref(b), C.byref(f), int(reset)))
        return ms, b.value, f.value


class MultiStream:
    """ONE stream over several devices (orbfe_stream_multi_*): batch k goes to devices[k % n], pop() returns the batches strictly in
    push order.  `devices` may name a device several times."""

    def __init__(self, nfeatures, scale, nlevels, ini_th, min_th, devices, batch, depth=2):
        self.L = load_library()
        h = C.c_void_p()
        ids = (C.c_int * len(devices))(*devices)
        _check(self.L.orbfe_stream_multi_create(nfeatures, scale, nlevels, ini_th, min_th, ids, len(devices), batch, depth, C.byref(h)))
        self.h = h
        self.batch = batch
        self.devices = list(devices)
        self.cap = self.L.orbfe_stream_multi_capacity(h)

    def close(self):
        if getattr(self, 'h', None):
            self.L.orbfe_stream_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_matching(self, bounds, window=100, nnratio=0.9, check_ori=True):
        b = np.asarray(bounds, np.float32)
        _check(self.L.orbfe_stream_multi_set_matching(self.h, _p(b), window, nnratio, int(check_ori)))

    def set_blur_variant(self, variant):
        _check(self.L.orbfe_stream_multi_set_blur_variant(self.h, int(variant)))

    def set_camera(self, fx, fy, cx, cy, dist=(), mode=0):
        """orbfe_stream_multi_set_camera: every runner and the boundary pairs match on mvKeysUn; only while no batch is in flight."""
        d = np.ascontiguousarray(dist, np.float32)
        _check(self.L.orbfe_stream_multi_set_camera(self.h, mode, fx, fy, cx, cy, _p(d) if len(d) else None, len(d)))

    def set_camera_equidistant(self, fx, fy, cx, cy):
        """orbfe_stream_multi_set_camera_equidistant: the fisheye model for every runner."""
        _check(self.L.orbfe_stream_multi_set_camera_equidistant(self.h, fx, fy, cx, cy))

    def equidistant_stats(self):
        out = np.zeros(3, np.int64)
        _check(self.L.orbfe_stream_multi_equidistant_stats(self.h, _p(out)))
        return out

    def xy_un(self):
        """mvKeysUn [B, cap, 2] of the last popped batch (a copy)."""
        p = C.c_void_p()
        _check(self.L.orbfe_stream_multi_xy_un(self.h, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(self.batch, self.cap, 2)).copy()

    def device_of_next_push(self):
        return int(self.L.orbfe_stream_multi_device_of_next_push(self.h))

    def push_ptrs(self, ptrs, rows, cols, stride, on_device=True):
        assert len(ptrs) == self.batch
        arr = (C.c_void_p * self.batch)(*ptrs)
        _check(self.L.orbfe_stream_multi_push(self.h, arr, int(on_device), rows, cols, stride))
        self.cap = self.L.orbfe_stream_multi_capacity(self.h)

    def pop(self, copy=False):
        """-> (kps[B,cap], desc[B,cap,32], n[B], matches12[B,cap], nmatches[B]) as views valid until the next pop."""
        pk, pd, pn, pm, pnm = (C.c_void_p() for _ in range(5))
        _check(self.L.orbfe_stream_multi_pop(self.h, C.byref(pk), C.byref(pd), C.byref(pn), C.byref(pm), C.byref(pnm)))
        return _result_views(self.batch, self.cap, (pk, pd, pn, pm, pnm), copy)
