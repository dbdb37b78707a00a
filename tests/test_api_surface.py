"""The Python surface of `api`, the package's one public namespace: every public class, function and public method (with __init__),
whichever module of the package defines it, against a literal table - names, order, kinds and defaults of the parameters, spelled as
test_matcher_surface.spelled does.  The table was generated once, at the commit before the handle classes moved out of api.py, by

    import pprint; from so_dso_place_recognition_amd import api; from test_api_surface import surface
    fns, cls = surface(api)
    print("FUNCTIONS =", pprint.pformat(fns, width=150)); print("CLASSES =", pprint.pformat(cls, width=150))

and is kept as a literal: a signature that changes, a name that disappears from api or a new public one fails here.  Also: the private
names tests and tools reach through api, and that importing api does not import torch.  Needs no GPU."""
import inspect
import os
import subprocess
import sys

import pytest

from so_dso_place_recognition_amd import api
from test_matcher_surface import spelled


def surface(api):
    """({function: parameters}, {class: {method: parameters}}) of the public names of `api` that the package defines"""
    pub = {n: o for n, o in vars(api).items() if not n.startswith("_") and getattr(o, "__module__", "").startswith(api.__package__)}
    members = lambda c: {m: getattr(c, m) for m in dir(c) if m == "__init__" or not m.startswith("_")}
    return ({n: spelled(o) for n, o in sorted(pub.items()) if inspect.isfunction(o)},
            {n: {m: spelled(f) for m, f in members(o).items() if inspect.isfunction(f) or inspect.ismethod(f)} for n, o in sorted(pub.items()) if inspect.isclass(o)})


FUNCTIONS = {'bow_distance_f64': 'hist1, hist2, ctx=None',
 'bow_generate': 'descriptors, vocab, cols=4000, ctx=None, return_counts=False',
 'bow_generate_torch': 'desc, offs, vocab, cols=4000, ctx=None, out=None, n_words=None, feature_words=None',
 'bow_match_topk': 'hist1, hist2, mask_width=0, k=1, ctx=None',
 'cloud_frames': 'xyz, inten, offs, ctx=None',
 'default_context': '',
 'delight_distance_f64': 'hist1, hist2, ctx=None',
 'delight_generate': 'xyz, inten, offs, ctx=None',
 'delight_match_topk': 'hist1, hist2, mask_width=0, k=1, ctx=None',
 'gist_distance_f64': 'hist1, hist2, ctx=None',
 'gist_generate': 'images, nblocks=4, orients=(8, 8, 8, 8), ctx=None',
 'gist_generate_torch': 'images, nblocks=4, orients=(8, 8, 8, 8), ctx=None, out=None',
 'gist_match_topk': 'hist1, hist2, mask_width=0, k=1, ctx=None',
 'gist_signature_size': 'nblocks=4, orients=(8, 8, 8, 8)',
 'hash_order': 'keys',
 'icp_accept': 'stats, min_fitness, max_rmse',
 'icp_nn': 'xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T, ctx=None',
 'icp_nn_radius': 'xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T, max_corr=1.0, ctx=None, search=None',
 'icp_refine': 'xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T0, max_iter=30, max_corr=1.0, tol_rmse=1e-06, tol_fitness=1e-06, min_inliers=3, '
               'ctx=None, search=None',
 'icp_refine_torch': 'xyz_q, offs_q, xyz_db, offs_db, pair_src, pair_dst, T0, max_src_pts, max_dst_pts, max_iter=30, max_corr=1.0, tol_rmse=1e-06, '
                     'tol_fitness=1e-06, min_inliers=3, ctx=None, out=None, search=None',
 'icp_search': 'ctx, search',
 'icp_tile_rows': '',
 'm2dp_generate': 'xyz, inten, offs, max_rho=45.0, ctx=None',
 'm2dp_svd_rows': 'ctx=None',
 'match_align': 'type_, hist1, hist2, idx, ctx=None',
 'match_align_fused': 'sc1, m2dp1, sc2, m2dp2, idx, ctx=None',
 'match_topk': 'type_, hist1, hist2, mask_width=0, p_weight=2.0, k=1, ctx=None',
 'match_topk_fused': 'sc1, m2dp1, sc2, m2dp2, mask_width=0, p_weight=2.0, k=1, ctx=None',
 'match_topk_seq': 'type_, hist1, hist2, steps, mask_width=0, p_weight=2.0, k=1, ctx=None',
 'processBoW': 'hist1, hist2, ctx=None',
 'processDELIGHT': 'hist1, hist2, ctx=None',
 'processGIST': 'hist1, hist2, ctx=None',
 'processM2DP': 'hist1, hist2, ctx=None',
 'processSC': 'hist1, hist2, ctx=None',
 'pts_preprocess': 'poses_file, pts_file, incoming_id_file, lidarRange=45.0, polar_filter=False, verbose=False, gpu=False, ctx=None',
 'read_poses_points': 'poses_file, pts_file',
 'read_signatures': 'path',
 'relative_pose': 'type_, frames_q, frames_db, variant',
 'relative_pose_torch': 'type_, frames_q, frames_db, idx, variant, hypotheses=1, db_row0=0, ctx=None',
 'run_test': 'type_, hist1, hist2, gt1=None, gt2=None, loop_diff=None, mask_width=0, ctx=None, device_eval=False',
 'sc_generate': 'xyz, inten, offs, max_rho=45.0, ctx=None',
 'sc_relative_pose': 'frames_q, frames_db, variant',
 'seq_select_torch': 'd_p, d_i, mom, steps, q_row0=0, db_row0=0, mask_width=0, p_weight=2.0, k=1, dense=False, ctx=None, out=None',
 'seq_steps': 'L, velocities',
 'seq_tile': '',
 'split_points_by_pose': 'pose_ids, point_ids',
 'verify_matches': 'clouds_q, clouds_db, idx, variant, frames_q, frames_db, max_corr=1.0, min_fitness=0.5, max_rmse=0.5, max_iter=30, '
                   'tol_rmse=1e-06, tol_fitness=1e-06, min_inliers=3, ctx=None, search=None',
 'verify_pairs_torch': 'type_, clouds_q, clouds_db, frames_q, frames_db, idx, variant, max_src_pts, max_dst_pts, hypotheses=1, db_row0=0, '
                       'max_corr=1.0, min_fitness=0.5, max_rmse=0.5, max_iter=30, tol_rmse=1e-06, tol_fitness=1e-06, min_inliers=3, ctx=None, '
                       'out=None, search=None',
 'write_points': 'path, ids, xyz, inten',
 'write_poses': 'path, ids, w2c',
 'write_signatures': "path, sig, dtype=<class 'numpy.float64'>"}
CLASSES = {'AteStats': {},
 'ClosureGate': {'__init__': 'self, ctx, pg_src, pg_dst, max_gap, min_support=2, rounds=8, rot_deg=2.0, rot_deg_per_kf=0.05, trans=0.5, '
                             'trans_per_kf=0.02, rot_tab=None, trans2_tab=None',
                 'close': 'self',
                 'run': 'self, poses, n',
                 'run_map': 'self, km, **kw',
                 'run_torch': 'self, poses, n, keep=None, support=None, map=None, info=None'},
 'CloudWindow': {'__init__': 'self, ctx=None, lidar_range=45.0, polar=False, point_capacity=1048576, max_new=65536, max_out=131072',
                 'close': 'self',
                 'count': 'self',
                 'empty_out': 'self, device=None',
                 'push': 'self, pose, xyz, inten',
                 'push_torch': 'self, pose, xyz, inten, n_new, out=None',
                 'reset': 'self'},
 'Context': {'__init__': 'self, device=0, sc_arith=None, stream=None, nan_policy=None, exact_statistics=None, sc_binary=None',
             'check': 'self, rc',
             'close': 'self',
             'kernel_timing': 'self, on',
             'last_distance_timing': 'self',
             'sync': 'self',
             'take_warnings': 'self'},
 'DELIGHT': {'__init__': 'self, ctx=None', 'getSignature': 'self, pts, intensity', 'getSignatureSize': 'self'},
 'GIST': {'__init__': 'self, params=None, ctx=None', 'extract': 'self, img', 'getSignatureSize': 'self'},
 'GISTParams': {},
 'Group': {'__init__': 'self, devices',
           'append_database': 'self, hist_new',
           'close': 'self',
           'last_timing': 'self',
           'match_topk': 'self, hist1, mask_width=0, p_weight=2.0, k=1',
           'set_database': 'self, type_, hist2, extra_capacity=0',
           'set_timing': 'self, on',
           'take_warnings': 'self'},
 'KeyframeMap': {'__init__': 'self, ctx, keyframe_capacity, point_capacity, max_cloud_points, max_append=1, buffers=None',
                 'append': 'self, xyz, inten, offs, frames, poses=None, ids=None, emitted=None',
                 'append_push': 'self, out, pose=None, id=None, info=None',
                 'append_torch': 'self, xyz, inten, offs, frames, poses=None, ids=None, emitted=None, max_points=None, info=None',
                 'close': 'self',
                 'count': 'self',
                 'reset': 'self',
                 'verify_dev': 'self, matcher, idx, clouds_q, frames_q, max_src_pts, hypotheses=1, seed=None, max_corr=1.0, min_fitness=0.5, '
                               'max_rmse=0.5, max_iter=30, tol_rmse=1e-06, tol_fitness=1e-06, min_inliers=3, out=None, search=None',
                 'verify_variants': 'self, type_, idx, variant, clouds_q, frames_q, max_src_pts, hypotheses=1, max_corr=1.0, min_fitness=0.5, '
                                    'max_rmse=0.5, max_iter=30, tol_rmse=1e-06, tol_fitness=1e-06, min_inliers=3, out=None, search=None'},
 'M2DP': {'__init__': 'self, max_rho, ctx=None', 'getSignatureSize': 'self', 'getSignatures': 'self, pts, intensity'},
 'MapGrower': {'__init__': 'self, ctx, wm, ml',
               'close': 'self',
               'count': 'self',
               'extend': 'self, row, poses=None',
               'extend_torch': 'self, row, poses=None, info=None',
               'normals': 'self, radius, min_nbrs, max_ratio, normals, ninfo',
               'normals_torch': 'self, radius, min_nbrs, max_ratio, normals, ninfo',
               'rebuild_torch': 'self, plane, poses=None, n=None, radius=0.4, min_nbrs=5, max_ratio=0.1, out=None, infos=None',
               'sync_torch': 'self, n=None'},
 'MapLocalizer': {'__init__': 'self, ctx, wm, cell, pair_capacity, max_src_pts',
                  'close': 'self',
                  'count': 'self',
                  'index': 'self',
                  'index_torch': 'self, info=None',
                  'localize_torch': 'self, xyz_q, offs_q, poses, n, idx, accepted=None, T_rel=None, src=None, excl=None, max_iter=30, max_corr=0.9, '
                                    'tol_rmse=1e-06, tol_fitness=1e-06, min_inliers=3, min_fitness=0.5, max_rmse=0.5, out=None',
                  'nn': 'self, xyz_q, offs_q, pair_src, T, excl=None, max_corr=0.9',
                  'nn_torch': 'self, xyz_q, offs_q, pair_src, T, excl=None, max_corr=0.9, out=None',
                  'refine': 'self, xyz_q, offs_q, pair_src, T0, excl=None, max_iter=30, max_corr=0.9, tol_rmse=1e-06, tol_fitness=1e-06, '
                            'min_inliers=3',
                  'refine_torch': 'self, xyz_q, offs_q, pair_src, T0, excl=None, max_iter=30, max_corr=0.9, tol_rmse=1e-06, tol_fitness=1e-06, '
                                  'min_inliers=3, out=None',
                  'seed_torch': 'self, poses, n, idx, accepted=None, T_rel=None, src=None, out=None'},
 'ORBVocabulary': {'__init__': 'self, path=None',
                   'arrays': 'self',
                   'close': 'self',
                   'empty': 'self',
                   'from_arrays': 'k, L, scoring, weighting, parent, is_leaf, desc, weight',
                   'info': 'self',
                   'loadFromTextFile': 'self, path',
                   'save': 'self, path',
                   'size': 'self',
                   'transform': 'self, descriptors, ctx=None'},
 'OnlineDatabase': {'__init__': 'self, ctx, type_, capacity, max_k=8, buffers=None',
                    'align': 'self, idx, sig, out=None',
                    'append': 'self, sig',
                    'append_torch': 'self, sig, emitted=None, info=None',
                    'close': 'self',
                    'count': 'self',
                    'match_torch': 'self, sig, mask_width=0, p_weight=2.0, k=1, emitted=None, out=None, rows=None',
                    'reset': 'self',
                    'step_torch': 'self, sig, mask_width=0, p_weight=2.0, k=1, emitted=None, out=None, rows=None, info=None'},
 'OnlineSet': {'__init__': 'self, ctx, kind, capacity, max_k=8, buffers=None',
               'align': 'self, idx, sigs, out=None',
               'append': 'self, sigs',
               'append_torch': 'self, sigs, emitted=None, info=None',
               'close': 'self',
               'count': 'self',
               'match_torch': 'self, sigs, mask_width=0, p_weight=2.0, k=1, emitted=None, out=None, rows=None',
               'reset': 'self',
               'step_torch': 'self, sigs, mask_width=0, p_weight=2.0, k=1, emitted=None, out=None, rows=None, info=None'},
 'PRError': {'__init__': 'self, code, msg'},
 'PlaneLocalizer': {'__init__': 'self, ctx, ml',
                    'close': 'self',
                    'localize_torch': 'self, xyz_q, offs_q, poses, n, idx, normals, ninfo, accepted=None, T_rel=None, src=None, excl=None, '
                                      'max_iter=30, max_corr=0.9, tol_rmse=1e-06, tol_fitness=1e-06, min_inliers=6, min_fitness=0.5, max_rmse=0.5, '
                                      'out=None',
                    'normals': 'self, radius, min_nbrs=5, max_ratio=0.1',
                    'normals_torch': 'self, radius, min_nbrs=5, max_ratio=0.1, out=None',
                    'refine': 'self, xyz_q, offs_q, pair_src, T0, normals, ninfo, excl=None, max_iter=30, max_corr=0.9, tol_rmse=1e-06, '
                              'tol_fitness=1e-06, min_inliers=6',
                    'refine_torch': 'self, xyz_q, offs_q, pair_src, T0, normals, ninfo, excl=None, max_iter=30, max_corr=0.9, tol_rmse=1e-06, '
                                    'tol_fitness=1e-06, min_inliers=6, out=None'},
 'PoseGraph': {'__init__': 'self, ctx, node_capacity, edge_capacity, max_outer=10, max_inner=256, buffers=None',
               'add': 'self, idx, T, accepted, query_row, w_rot=1.0, w_trans=1.0',
               'add_batch': 'self, i, j, T, accepted, w=None, w_rot=1.0, w_trans=1.0',
               'add_batch_torch': 'self, i, j, T, accepted, w=None, w_rot=1.0, w_trans=1.0, info=None',
               'add_torch': 'self, idx, T, accepted, query_row, w_rot=1.0, w_trans=1.0, info=None',
               'add_weighted': 'self, idx, T, accepted, query_row, w',
               'add_weighted_torch': 'self, idx, T, accepted, query_row, w, info=None',
               'close': 'self',
               'count': 'self',
               'relax_map': 'self, km, **kw',
               'relax_torch': 'self, poses, n, outer=5, inner=64, lam=1e-09, w_odo_rot=1.0, w_odo_trans=1.0, out=None, report=None',
               'reset': 'self'},
 'Proximity': {},
 'ProximitySearch': {'__init__': 'self, ctx, node_capacity, query_capacity, k_max',
                     'close': 'self',
                     'scratch_bytes': 'self',
                     'search': 'self, poses, n, qrange, kwonly:radius, kwonly:growth=0.0, kwonly:radius_max=None, kwonly:cos_min=-1.0, '
                               'kwonly:min_gap, kwonly:stride=1, kwonly:k=1, kwonly:log=None, kwonly:known_window=0',
                     'search_map': 'self, km, qrange, **kw',
                     'search_torch': 'self, poses, n, qrange, kwonly:radius, kwonly:growth=0.0, kwonly:radius_max=None, kwonly:cos_min=-1.0, '
                                     'kwonly:min_gap, kwonly:stride=1, kwonly:k=1, kwonly:log=None, kwonly:known_window=0, kwonly:out=None',
                     'shapes': 'self, k',
                     'tile': '',
                     'verify_map_torch': 'self, km, cand, max_src_pts, kwonly:max_iter=30, kwonly:max_corr=1.0, kwonly:min_fitness=0.5, '
                                         'kwonly:max_rmse=0.5, kwonly:tol_rmse=1e-06, kwonly:tol_fitness=1e-06, kwonly:min_inliers=3, '
                                         'kwonly:search=None, kwonly:out=None'},
 'RegInfo': {},
 'RegistrationInfo': {'__init__': 'self, ctx, pair_capacity, max_src_pts',
                      'close': 'self',
                      'maploc_torch': 'self, plane_localizer, xyz_q, offs_q, pair_src, T, normals, ninfo, accepted=None, excl=None, max_corr=0.9, '
                                      'min_inliers=10, min_ratio=0.0001, sigma_min=0.01, w_max=1000000.0, out=None',
                      'pairs_torch': 'self, clouds_q, clouds_db, idx, T, accepted, max_src_pts, max_dst_pts, max_corr=1.0, min_inliers=10, '
                                     'min_ratio=0.0001, sigma_min=0.01, w_max=1000000.0, out=None',
                      'plane': 'self, xyz_q, offs_q, pair_src, T, nn, world_xyz, normals, ninfo, accepted=None, max_corr=0.9, min_inliers=10, '
                               'min_ratio=0.0001, sigma_min=0.01, w_max=1000000.0',
                      'plane_torch': 'self, xyz_q, offs_q, pair_src, T, nn, world_xyz, normals, ninfo, accepted=None, max_corr=0.9, min_inliers=10, '
                                     'min_ratio=0.0001, sigma_min=0.01, w_max=1000000.0, out=None',
                      'point': 'self, xyz_q, offs_q, pair_src, T, nn, accepted=None, max_corr=1.0, min_inliers=10, min_ratio=0.0001, sigma_min=0.01, '
                               'w_max=1000000.0',
                      'point_torch': 'self, xyz_q, offs_q, pair_src, T, nn, accepted=None, max_corr=1.0, min_inliers=10, min_ratio=0.0001, '
                                     'sigma_min=0.01, w_max=1000000.0, out=None'},
 'SC': {'__init__': 'self, max_rho, ctx=None', 'getSignature': 'self, pts, intensity', 'getSignatureSize': 'self'},
 'SequenceFilter': {'__init__': 'self, ctx, capacity, channels, steps, max_k=8',
                    'close': 'self',
                    'push': 'self, rows, count, weights, normalize=True, mask_width=0, k=1',
                    'push_torch': 'self, rows, state, weights, normalize=True, mask_width=0, k=1, emitted=None, out=None',
                    'read': 'self',
                    'reset': 'self'},
 'SubmapBuilder': {'__init__': 'self, ctx, slot_capacity, w_max, point_capacity, max_cloud_points, keyframe_capacity=None, buffers=None',
                   'build': 'self, km, centers, avoid=None, poses=None, n=None, kwonly:w, kwonly:past_only=False, kwonly:avoid_gap=0, '
                            'kwonly:max_pts=None',
                   'build_torch': 'self, km, centers, avoid=None, poses=None, n=None, kwonly:w, kwonly:past_only=False, kwonly:avoid_gap=0, '
                                  'kwonly:max_pts=None, kwonly:out=None',
                   'close': 'self',
                   'new_out': 'self',
                   'pair_torch': 'self, km, idx_db, idx_q, poses=None, n=None, kwonly:w, kwonly:avoid_gap=0, kwonly:max_pts=None, kwonly:out=None',
                   'scratch_bytes': 'self',
                   'shapes': 'self'},
 'Submaps': {},
 'TrajEval': {},
 'TrajectoryEval': {'__init__': "self, ctx, node_capacity, B=1, align='sim3', gt_kind='c2w', deltas=(1, 10), lengths=(100.0, 200.0, 300.0, 400.0, "
                                '500.0, 600.0, 700.0, 800.0), step=1, edge_capacity=0, rot_thr=0.08726646259971647, trans_thr=2.0',
                    'ate_stats': 'ate',
                    'close': 'self',
                    'run': "self, est, n, gt, valid=None, log=None, optional=('err', 'seg_end', 'edge_err', 'centres', 'prefix')",
                    'run_map': 'self, km, gt, poses=None, **kw',
                    'run_torch': "self, est, n, gt, valid=None, log=None, out=None, optional=('err', 'seg_end', 'edge_err')",
                    'scratch_bytes': 'self',
                    'shapes': 'self, log=True'},
 'WorldMap': {'__init__': 'self, ctx, km, out_capacity, buffers=None',
              'close': 'self',
              'count_rows': 'self',
              'fuse': "self, poses=None, n=None, cell=0.2, min_count=1, keep='first'",
              'fuse_torch': "self, poses=None, n=None, cell=0.2, min_count=1, keep='first', info=None",
              'rows': 'self',
              'write_ply': 'self, path, binary=True'}}


def test_public_functions_take_what_they_took():
    assert surface(api)[0] == FUNCTIONS


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_public_methods_take_what_they_took(cls):
    assert surface(api)[1][cls] == CLASSES[cls]


def test_no_public_class_came_or_went():
    assert sorted(surface(api)[1]) == sorted(CLASSES)


def test_private_names_tests_and_tools_use():
    for name in ("_ptr", "_csr", "_lib", "_pts_preprocess_stream"):
        assert hasattr(api, name), name


def test_importing_api_does_not_import_torch():
    code = "import sys; from so_dso_place_recognition_amd import api; sys.exit(1 if 'torch' in sys.modules else 0)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0          # a fresh interpreter: this one has torch
