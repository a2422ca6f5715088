"""Host mirrors of the back end: the scan-to-submap optimisation (reference src/backMapping.cpp:681-1058) over rolo_scan2map_optimize, the
device-resident key frames with sub-map assembly (:558-678) over rolo_keymap_*, Scan Context loop detection (src/scancontext/Scancontext.cpp) over
rolo_keymap_sc_*, the loop closure's clouds, radius-search detector and ICP (:2307-2624) over rolo_keymap_loop_* / rolo_loopicp_*, the factor graph
(:1222-1320) as a batch pose-graph optimisation over rolo_pgo_*, and the clouds of the exports (publishGlobalMap :1611-1665, cloudGlobal.pcd :1546-1557) over
rolo_keymap_global_*, and the ground prior (src/prior_pose/pose_solver.cpp, prior_pose_node.cpp:164-233) over rolo_ground_* / rolo_priorpose_*; and the node's
per-scan step laserCloudInfoHandler (:420-457) as one call over all of them: MapOptimization over rolo_mapper_*."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, check, Scan2MapStats, ScParams, ScResult, LoopIcpParams, LoopIcpResult, LoopIcpTraceRec, PgoParams, PgoResult, PgoTraceRec, PriorPoseParams, PriorPoseResult, PriorPoseFit, MapperParams, MapperResult
from .rotvgicp import RotVGICP


class Scan2Map:
    def __init__(self, device: int = 0, edgeFeatureMinValidNum: int = 10, surfFeatureMinValidNum: int = 100):
        self.reg = RotVGICP(device)   # a context of its own: its clouds hold the sub-map trees
        self.edge_min, self.surf_min = edgeFeatureMinValidNum, surfFeatureMinValidNum
        self.last_stats = None

    def close(self):
        self.reg.close()

    def setSubmap(self, map_corner, map_surf):
        """kdtree*FromMap->setInputCloud (:690-691): the sub-map stays resident; scan2MapOptimization(corner, surf, None, None, tf) registers against it"""
        fp = C.POINTER(C.c_float)
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 4) for x in (map_corner, map_surf)]
        check(lib().rolo_scan2map_set_submap(self.reg._h, a[0].ctypes.data_as(fp), a[0].shape[0], a[1].ctypes.data_as(fp), a[1].shape[0]), "rolo_scan2map_set_submap")

    def setSubmapFrom(self, keymap: "KeyFrameMap"):
        """setSubmap on the key map's last extractCloud, device to device"""
        check(lib().rolo_scan2map_set_submap_keymap(self.reg._h, keymap._h), "rolo_scan2map_set_submap_keymap")

    def scan2MapOptimization(self, corner, surf, map_corner, map_surf, transformTobeMapped, want_debug=False):
        """Returns the updated transformTobeMapped (roll, pitch, yaw, x, y, z; float32) [, selected flags, coeffSel of the last iteration].
        map_corner = map_surf = None: the resident sub-map of setSubmap."""
        fp = C.POINTER(C.c_float)
        if map_corner is None and map_surf is None:
            map_corner = map_surf = np.zeros((0, 4), np.float32)
            resident = True
        else:
            resident = False
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 4) for x in (corner, surf, map_corner, map_surf)]
        tf = np.ascontiguousarray(transformTobeMapped, np.float32).copy()
        st = Scan2MapStats()
        n = a[0].shape[0] + a[1].shape[0]
        sel = np.zeros(max(n, 1), np.uint8) if want_debug else None
        coeff = np.zeros((max(n, 1), 4), np.float32) if want_debug else None
        check(lib().rolo_scan2map_optimize(self.reg._h, a[0].ctypes.data_as(fp), a[0].shape[0], a[1].ctypes.data_as(fp), a[1].shape[0], None if resident else a[2].ctypes.data_as(fp), a[2].shape[0],
                                           None if resident else a[3].ctypes.data_as(fp), a[3].shape[0], tf.ctypes.data_as(fp), self.edge_min, self.surf_min, C.byref(st),
                                           sel.ctypes.data_as(C.POINTER(C.c_ubyte)) if want_debug else None, coeff.ctypes.data_as(fp) if want_debug else None),
              "rolo_scan2map_optimize")
        self.last_stats = st
        return (tf, sel[:n].astype(bool), coeff[:n]) if want_debug else tf


def select_nearby(xyz, times, time_cur, search_radius=50.0, density=2.0, recent_seconds=10.0):
    """extractNearby (:575-614) with extractCloud's range filter (:626): the key-frame indices extractCloud would fuse, in its order (host only)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    times = np.ascontiguousarray(times, np.float64).reshape(-1)
    assert times.shape[0] == xyz.shape[0]
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = np.zeros(max(2 * xyz.shape[0], 1), np.int32)   # at most one entry per radius hit and one per recent pose
    m = check(lib().rolo_keyposes_select_nearby(xyz.ctypes.data_as(fp), times.ctypes.data_as(dp), xyz.shape[0], search_radius, density, time_cur, recent_seconds,
                                                out.ctypes.data_as(ip), out.shape[0]), "rolo_keyposes_select_nearby")
    assert m <= out.shape[0]
    return out[:m].copy()


def select_global(xyz, search_radius=1000.0, pose_density=10.0):
    """publishGlobalMap's selection (:1619-1654): select_nearby's radius search, pose filter and range test with no key pose admitted by its time (the reference
    has no "recent" clause here); host only"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return select_nearby(xyz, np.zeros(xyz.shape[0]), 0.0, search_radius, pose_density, -np.inf)


def detect_loop_distance(xyz, times, time_cur, search_radius=30.0, time_diff=30.0) -> int:
    """detectLoopClosureDistance (:2481-2515) without its loopIndexContainer test: the nearest key pose within search_radius of the last one that is more than
    time_diff away from time_cur, or -1 (none, or the last key itself); host only"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    times = np.ascontiguousarray(times, np.float64).reshape(-1)
    assert times.shape[0] == xyz.shape[0]
    pre = C.c_int32(-1)
    check(lib().rolo_keyposes_detect_loop_distance(xyz.ctypes.data_as(C.POINTER(C.c_float)), times.ctypes.data_as(C.POINTER(C.c_double)), xyz.shape[0],
                                                   search_radius, time_diff, time_cur, C.byref(pre)), "rolo_keyposes_detect_loop_distance")
    return pre.value


def loop_icp_params(max_correspondence_distance=np.inf, **kw) -> LoopIcpParams:
    """the reference's ICP settings (:2342-2346): 100 iterations, both epsilons 1e-6; fields of rolo_loopicp_params by keyword"""
    p = LoopIcpParams()
    lib().rolo_loopicp_default_params(C.byref(p))
    p.max_correspondence_distance = max_correspondence_distance
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _icp_result(res: LoopIcpResult) -> dict:
    return dict(T=np.array(res.T, np.float32).reshape(4, 4), fitness=res.fitness, converged=bool(res.converged), iterations=res.iterations, state=res.state,
                n_source=res.n_source, n_target=res.n_target, n_last=res.n_last)


def _icp_trace(fn, handle):
    n = check(fn(handle, None, 0), "loop ICP trace")
    recs = (LoopIcpTraceRec * max(n, 1))()
    check(fn(handle, recs, n), "loop ICP trace")
    return [dict(n=r.n, mse=r.mse, sums=np.array(r.sums, np.float64), increment=np.array(r.increment, np.float32).reshape(4, 4)) for r in recs[:n]]


def _guess_ptr(guess):
    if guess is None:
        return None, None
    g = np.ascontiguousarray(guess, np.float32).reshape(16)
    return g, g.ctypes.data_as(C.POINTER(C.c_float))


class LoopIcp:
    """pcl::IterativeClosestPoint as the loop closure configures it, on two host clouds (n x 4 floats): the route for users without a key map, and the tests'"""
    STATES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")

    def __init__(self, device: int = 0):
        self.reg = RotVGICP(device)   # a context of its own: its clouds hold the target's tree

    def close(self):
        self.reg.close()

    def align(self, source, target, params: LoopIcpParams = None, guess=None) -> dict:
        fp = C.POINTER(C.c_float)
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 4) for x in (source, target)]
        res = LoopIcpResult()
        keep, g = _guess_ptr(guess)
        check(lib().rolo_loopicp_align(self.reg._h, a[0].ctypes.data_as(fp), a[0].shape[0], a[1].ctypes.data_as(fp), a[1].shape[0],
                                       C.byref(params if params is not None else loop_icp_params()), g, C.byref(res)), "rolo_loopicp_align")
        return _icp_result(res)

    def trace(self):
        """one record per association of the last align, the fitness pass last"""
        return _icp_trace(lib().rolo_loopicp_get_trace, self.reg._h)

    def associate(self, source, target, T=None, max_correspondence_distance=np.inf):
        """test hook: (target index, d2) of every source point moved by T, -1 / inf beyond the cap"""
        fp = C.POINTER(C.c_float)
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 4) for x in (source, target)]
        idx = np.zeros(a[0].shape[0], np.int32); d2 = np.zeros(a[0].shape[0], np.float32)
        keep, g = _guess_ptr(T)
        check(lib().rolo_loopicp_associate(self.reg._h, a[0].ctypes.data_as(fp), a[0].shape[0], a[1].ctypes.data_as(fp), a[1].shape[0], g, max_correspondence_distance,
                                           idx.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(fp)), "rolo_loopicp_associate")
        return idx, d2

    def lastMs(self):
        """device milliseconds of the last align: set-up, iterations, fitness pass, whole call"""
        ms = np.zeros(4, np.float32)
        check(lib().rolo_loopicp_last_ms(self.reg._h, ms.ctypes.data_as(C.POINTER(C.c_float))), "rolo_loopicp_last_ms")
        return ms

    MAX_BATCH = 256   # ROLO_LOOPICP_MAX_BATCH

    def alignBatch(self, sources, target, params: LoopIcpParams = None, guesses=None) -> list:
        """align(sources[b], target, params, guesses[b]) for every b, bit for bit, with all candidates' associations in one launch per iteration"""
        fp = C.POINTER(C.c_float)
        srcs = [np.ascontiguousarray(x, np.float32).reshape(-1, 4) for x in sources]
        B = len(srcs)
        tgt = np.ascontiguousarray(target, np.float32).reshape(-1, 4)
        cat = np.ascontiguousarray(np.concatenate(srcs, 0) if B else np.zeros((0, 4), np.float32))
        ns = np.array([s.shape[0] for s in srcs], np.int32)
        g = None
        if guesses is not None:
            g = np.ascontiguousarray(guesses, np.float32).reshape(B, 16)
        res = (LoopIcpResult * max(B, 1))()
        check(lib().rolo_loopicp_align_batch(self.reg._h, cat.ctypes.data_as(fp), ns.ctypes.data_as(C.POINTER(C.c_int)), B, tgt.ctypes.data_as(fp), tgt.shape[0],
                                             C.byref(params if params is not None else loop_icp_params()), g.ctypes.data_as(fp) if g is not None else None, res),
              "rolo_loopicp_align_batch")
        return [_icp_result(res[b]) for b in range(B)]

    def traceBatch(self, b: int):
        """candidate b's records of the last alignBatch, as trace()"""
        return _icp_trace(lambda h, out, cap: lib().rolo_loopicp_get_trace_batch(h, b, out, cap), self.reg._h)

    def batchLastMs(self):
        """device milliseconds of the last alignBatch: set-up, iterations with the fitness passes, 0, whole call"""
        ms = np.zeros(4, np.float32)
        check(lib().rolo_loopicp_batch_last_ms(self.reg._h, ms.ctypes.data_as(C.POINTER(C.c_float))), "rolo_loopicp_batch_last_ms")
        return ms


class KeyFrameMap:
    """cornerCloudKeyFrames / surfCloudKeyFrames / cloudKeyPoses6D on the device, with extractSurroundingKeyFrames and downsampleCurrentScan"""

    def __init__(self, device: int = 0, mappingCornerLeafSize: float = 0.2, mappingSurfLeafSize: float = 0.4):
        self._h = C.c_void_p()
        check(lib().rolo_keymap_create(device, C.byref(self._h)), "rolo_keymap_create")
        self.corner_leaf, self.surf_leaf = mappingCornerLeafSize, mappingSurfLeafSize
        self.poses, self.times = [], []   # transformTobeMapped order: roll, pitch, yaw, x, y, z
        self._sizes = []                  # corner + surface points per key frame (sizes globalCloud's array)
        self.m_corner = self.m_surf = self.m_global = 0

    def close(self):
        if self._h:
            lib().rolo_keymap_destroy(self._h)
            self._h = C.c_void_p()

    def __len__(self):
        return check(lib().rolo_keymap_size(self._h), "rolo_keymap_size")

    def addKeyFrame(self, corner, surf, pose6, time: float) -> int:
        """saveKeyFramesAndFactor (:1140-1181): returns the key frame's index"""
        fp = C.POINTER(C.c_float)
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 4) for x in (corner, surf)]
        p = np.ascontiguousarray(pose6, np.float32).reshape(6)
        k = check(lib().rolo_keymap_add_keyframe(self._h, a[0].ctypes.data_as(fp), a[0].shape[0], a[1].ctypes.data_as(fp), a[1].shape[0], p.ctypes.data_as(fp), float(time)),
                  "rolo_keymap_add_keyframe")
        self.poses.append(p.copy()); self.times.append(float(time)); self._sizes.append(a[0].shape[0] + a[1].shape[0])
        return k

    def setPose(self, index: int, pose6):
        """correctPoses (:1301-1314)"""
        p = np.ascontiguousarray(pose6, np.float32).reshape(6)
        check(lib().rolo_keymap_set_pose(self._h, index, p.ctypes.data_as(C.POINTER(C.c_float))), "rolo_keymap_set_pose")
        self.poses[index] = p.copy()

    def setPoses(self, poses6):
        """correctPoses (:1301-1314) for key frames 0 .. n - 1 in one call"""
        p = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
        check(lib().rolo_keymap_set_poses(self._h, p.ctypes.data_as(C.POINTER(C.c_float)), p.shape[0]), "rolo_keymap_set_poses")
        for k in range(p.shape[0]):
            self.poses[k] = p[k].copy()

    def selectNearby(self, time_cur: float, search_radius: float = 50.0, density: float = 2.0, recent_seconds: float = 10.0):
        """extractNearby (:575-614) on the stored key poses"""
        xyz = np.array([p[3:6] for p in self.poses], np.float32).reshape(-1, 3)
        return select_nearby(xyz, self.times, time_cur, search_radius, density, recent_seconds)

    def extractCloud(self, indices):
        """extractCloud (:617-658): the two sub-maps stay on the device; returns their sizes"""
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        mc, ms = C.c_int(0), C.c_int(0)
        check(lib().rolo_keymap_extract(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.shape[0], self.corner_leaf, self.surf_leaf, C.byref(mc), C.byref(ms)),
              "rolo_keymap_extract")
        self.m_corner, self.m_surf = mc.value, ms.value
        return mc.value, ms.value

    def submap(self):
        """laserCloudCornerFromMapDS, laserCloudSurfFromMapDS of the last extractCloud (download)"""
        fp = C.POINTER(C.c_float)
        c = np.zeros((self.m_corner, 4), np.float32); s = np.zeros((self.m_surf, 4), np.float32)
        check(lib().rolo_keymap_get_submap(self._h, c.ctypes.data_as(fp), c.shape[0], s.ctypes.data_as(fp), s.shape[0]), "rolo_keymap_get_submap")
        return c, s

    def downsample(self, pts, leaf: float):
        """downSizeFilter*.filter of one cloud (downsampleCurrentScan :666-678)"""
        fp = C.POINTER(C.c_float)
        a = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        out = np.zeros_like(a)
        m = C.c_int(0)
        check(lib().rolo_keymap_downsample(self._h, a.ctypes.data_as(fp), a.shape[0], leaf, out.ctypes.data_as(fp), C.byref(m)), "rolo_keymap_downsample")
        return out[:m.value].copy()

    # ---- Scan Context (src/scancontext/Scancontext.cpp): descriptors of the key frames, resident beside their clouds ----
    def scParams(self) -> ScParams:
        """the defaults of Scancontext.h:80-95; change fields and hand the struct to scSetParams"""
        p = ScParams()
        lib().rolo_sc_default_params(C.byref(p))
        return p

    def scSetParams(self, p: ScParams):
        check(lib().rolo_keymap_sc_set_params(self._h, C.byref(p)), "rolo_keymap_sc_set_params")

    def scGetParams(self) -> ScParams:
        """the parameters the key map holds now"""
        p = ScParams()
        check(lib().rolo_keymap_sc_get_params(self._h, C.byref(p)), "rolo_keymap_sc_get_params")
        return p

    def scAddSurface(self, index: int) -> int:
        """scInputType scan_feat (backMapping.cpp:1213): the descriptor of key frame `index`'s resident surface cloud; returns the descriptor's index"""
        return check(lib().rolo_keymap_sc_add_surface(self._h, index), "rolo_keymap_sc_add_surface")

    def scAddCloud(self, pts, leaf: float = 0.5) -> int:
        """scInputType scan_raw (:1186-1196): downSizeFilterSC at `leaf` (0: none), then the descriptor; returns its index"""
        a = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        return check(lib().rolo_keymap_sc_add_cloud(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], leaf), "rolo_keymap_sc_add_cloud")

    def scSize(self) -> int:
        return check(lib().rolo_keymap_sc_size(self._h), "rolo_keymap_sc_size")

    def scDescriptor(self, i: int):
        """(desc num_ring x num_sector float64, ring key float32, sector key float64, column norms float64) of descriptor i"""
        p = self.scGetParams()   # the library's own geometry sizes the buffers it fills
        R, S = p.num_ring, p.num_sector
        desc = np.zeros((R, S), np.float64); ring = np.zeros(R, np.float32); sector = np.zeros(S, np.float64); norm = np.zeros(S, np.float64)
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        check(lib().rolo_keymap_sc_get(self._h, i, desc.ctypes.data_as(dp), ring.ctypes.data_as(fp), sector.ctypes.data_as(dp), norm.ctypes.data_as(dp)), "rolo_keymap_sc_get")
        return desc, ring, sector, norm

    def scDetect(self, query: int, n_search: int, want_candidates: bool = False):
        """detectLoopClosureID (:253-344) for descriptor `query` against descriptors 0 .. n_search-1 -> ScResult [, candidate indices, distances, alignments]"""
        res = ScResult()
        if not want_candidates:
            check(lib().rolo_keymap_sc_detect(self._h, query, n_search, C.byref(res), None, None, None, 0), "rolo_keymap_sc_detect")
            return res
        cap = max(n_search, 1)
        idx = np.zeros(cap, np.int32); dist = np.zeros(cap, np.float64); align = np.zeros(cap, np.int32)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        check(lib().rolo_keymap_sc_detect(self._h, query, n_search, C.byref(res), idx.ctypes.data_as(ip), dist.ctypes.data_as(dp), align.ctypes.data_as(ip), cap), "rolo_keymap_sc_detect")
        m = res.n_candidates
        return res, idx[:m].copy(), dist[:m].copy(), align[:m].copy()

    def scLastMs(self) -> float:
        return float(lib().rolo_keymap_sc_last_ms(self._h))

    # ---- loop closure (:2307-2624): the two loop clouds and their ICP, resident beside the key frames ----
    def loopCloud(self, slot: int, key: int, search_num: int, wrt_key: int = None, leaf: float = None) -> int:
        """loopFindNearKeyframes (:2572-2596), or ...WithRespectTo (:2598-2624) with wrt_key, into slot 0 (source) or 1 (target); returns the cloud's size"""
        m = C.c_int(0)
        check(lib().rolo_keymap_loop_cloud(self._h, slot, key, search_num, -1 if wrt_key is None else wrt_key, self.surf_leaf if leaf is None else leaf, C.byref(m)),
              "rolo_keymap_loop_cloud")
        return m.value

    def loopCloudPoints(self, slot: int, m: int):
        """download of a loop cloud (m: the size loopCloud returned)"""
        out = np.zeros((m, 4), np.float32)
        got = check(lib().rolo_keymap_get_loop_cloud(self._h, slot, out.ctypes.data_as(C.POINTER(C.c_float)), m), "rolo_keymap_get_loop_cloud")
        return out[:got].copy()

    def loopIcp(self, params: LoopIcpParams = None, guess=None) -> dict:
        """icp.align + getFitnessScore of slot 0 onto slot 1"""
        res = LoopIcpResult()
        keep, g = _guess_ptr(guess)
        check(lib().rolo_keymap_loop_icp(self._h, C.byref(params if params is not None else loop_icp_params()), g, C.byref(res)), "rolo_keymap_loop_icp")
        return _icp_result(res)

    def loopTrace(self):
        return _icp_trace(lib().rolo_keymap_loop_trace, self._h)

    def loopLastMs(self):
        """device milliseconds: ICP set-up, iterations, fitness pass, whole ICP call, assembly of slot 0, assembly of slot 1"""
        ms = np.zeros(6, np.float32)
        check(lib().rolo_keymap_loop_last_ms(self._h, ms.ctypes.data_as(C.POINTER(C.c_float))), "rolo_keymap_loop_last_ms")
        return ms

    def detect_loop_distance(self, time_cur: float, search_radius: float = 30.0, time_diff: float = 30.0) -> int:
        """detectLoopClosureDistance (:2481-2515) on the stored key poses"""
        xyz = np.array([p[3:6] for p in self.poses], np.float32).reshape(-1, 3)
        return detect_loop_distance(xyz, self.times, time_cur, search_radius, time_diff)

    # ---- the global map (publishGlobalMap :1611-1665, saveGlobalPCDs' cloudGlobal.pcd :1546-1557) ----
    def selectGlobal(self, search_radius: float = 1000.0, pose_density: float = 10.0):
        """the key frames publishGlobalMap fuses (:1619-1654), in its order: selectNearby's radius rule and pose filter, nothing admitted by time"""
        return select_global(np.array([p[3:6] for p in self.poses], np.float32).reshape(-1, 3), search_radius, pose_density)

    def globalMap(self, indices, leaf: float = 1.0, download: bool = True):
        """:1656-1663 — the listed key frames' clouds at their current poses through one VoxelGrid; the map stays on the device. Returns it (m x 4), or with
        download = False its size (globalMapPoints fetches it later)"""
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        m = C.c_int(0)
        check(lib().rolo_keymap_global_map(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.shape[0], leaf, C.byref(m)), "rolo_keymap_global_map")
        self.m_global = m.value
        return self.globalMapPoints() if download else m.value

    def globalMapPoints(self):
        """download of the last globalMap"""
        out = np.zeros((self.m_global, 4), np.float32)
        got = check(lib().rolo_keymap_get_global_map(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.shape[0]), "rolo_keymap_get_global_map")
        return out[:got]

    def globalCloud(self, indices):
        """:1546-1557 — the same clouds concatenated, unfiltered (cloudGlobal.pcd's points)"""
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
        total = sum(self._sizes[k] for k in idx.tolist()) if all(0 <= k < len(self._sizes) for k in idx.tolist()) else 0
        out = np.zeros((total, 4), np.float32)
        got = check(lib().rolo_keymap_global_cloud(self._h, ip, idx.shape[0], out.ctypes.data_as(C.POINTER(C.c_float)), total), "rolo_keymap_global_cloud")
        return out[:got]

    def setGlobalBatch(self, points: int):
        """points per batch of globalMap / globalCloud; 0: the library's default"""
        check(lib().rolo_keymap_global_set_batch(self._h, int(points)), "rolo_keymap_global_set_batch")

    def globalInfo(self) -> dict:
        """of the last globalMap: input points, batches, cells, the form that ran, the largest table size"""
        v = (C.c_longlong * 5)()
        check(lib().rolo_keymap_global_info(self._h, v, 5), "rolo_keymap_global_info")
        return dict(points=v[0], batches=v[1], cells=v[2], form=("one-shot", "streamed")[v[3]], table=v[4])

    def globalLastMs(self):
        """device milliseconds of the last globalMap: box pass, sort + merge pass, finish"""
        ms = np.zeros(3, np.float32)
        check(lib().rolo_keymap_global_last_ms(self._h, ms.ctypes.data_as(C.POINTER(C.c_float))), "rolo_keymap_global_last_ms")
        return ms

    def publishGlobalMap(self, search_radius: float = 1000.0, pose_density: float = 10.0, leaf: float = 1.0):
        """publishGlobalMap (:1611-1665) with config/params.yaml:67-69's defaults: selectGlobal, then globalMap"""
        return self.globalMap(self.selectGlobal(search_radius, pose_density), leaf)


class ScanContextManager:
    """SCManager's two user calls over a key map's descriptor store. detectLoopClosureID keeps the reference's rebuild-period counter and its stale searched set
    (Scancontext.cpp:263-282): the set is re-taken (all descriptors but the newest NUM_EXCLUDE_RECENT) only on every TREE_MAKING_PERIOD_-th call that gets past the
    early return, and calls in between search the set as it was."""
    TREE_MAKING_PERIOD = 10   # Scancontext.h:99

    def __init__(self, keymap: KeyFrameMap, params: ScParams = None, leaf: float = 0.0):
        self.km = keymap
        self.params = params if params is not None else keymap.scParams()
        keymap.scSetParams(self.params)
        self.leaf = leaf
        self.tree_making_period_counter = 0
        self.n_search = 0
        self.last = None

    def makeAndSaveScancontextAndKeys(self, scan_down) -> int:
        """:236-250 on a host cloud (n x 4 floats), already down-sampled as the reference's caller hands it over (leaf = 0) or filtered here at `leaf`"""
        return self.km.scAddCloud(scan_down, self.leaf)

    def makeAndSaveFromKeyFrame(self, index: int) -> int:
        """the same on key frame `index`'s resident surface cloud"""
        return self.km.scAddSurface(index)

    def detectLoopClosureID(self):
        """:253-344 -> (loop_id, yaw_diff_rad as np.float32); the query is the newest descriptor"""
        n = self.km.scSize()
        if n < self.params.num_exclude_recent + 1:   # :263-267
            self.last = None
            return -1, np.float32(0.0)
        if self.tree_making_period_counter % self.TREE_MAKING_PERIOD == 0:   # :270-281
            self.n_search = n - self.params.num_exclude_recent
        self.tree_making_period_counter += 1
        self.last = self.km.scDetect(n - 1, self.n_search)
        return self.last.loop_id, np.float32(self.last.yaw_diff_rad)


def pose6_to_T(pose6, dtype=np.float32):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) of a transformTobeMapped-order pose (roll, pitch, yaw, x, y, z), 4 x 4 in `dtype` arithmetic"""
    r, p, y, tx, ty, tz = (dtype(v) for v in pose6)
    A, B, Cc, D, E, F = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    DE, DF = D * E, D * F
    return np.array([[A * Cc, A * DF - B * E, B * F + A * DE, tx], [B * Cc, A * E + B * DF, B * DE - A * F, ty], [-D, Cc * F, Cc * E, tz], [0, 0, 0, 1]], dtype)


PGO_LOSS_CAUCHY = 1   # ROLO_PGO_LOSS_CAUCHY


class LoopFactor(tuple):
    """(loopKeyCur, loopKeyPre, poseFrom, poseTo, noise) as LoopCloser returns it, with the loss the reference wraps that noise in: `robust` is None (the plain
    diagonal of performRSLoopClosure, :2382-2385) or the Cauchy constant k (performSCLoopClosure's Robust noise with Cauchy(1), :2468-2470). It unpacks into the
    same five entries as the plain tuple."""
    def __new__(cls, entries, robust=None):
        self = super().__new__(cls, entries)
        self.robust = None if robust is None else float(robust)
        return self


class LoopCloser:
    """performRSLoopClosure (:2307-2397) and performSCLoopClosure (:2399-2479) over a key map, up to the factor graph: each call returns a LoopFactor
    (loopKeyCur, loopKeyPre, poseFrom 4 x 4, poseTo 4 x 4, noise) — the constraint is poseFrom.between(poseTo) with the variance `noise` on all six axes — or None.
    Its `robust` is None for the RS form and 1.0 for the SC form, whose noise the reference puts under a Cauchy(1) M-estimator because Scan Context can propose a
    wrong place. PoseGraph.addLoopFactor takes it as it is."""
    MIN_CUR, MIN_PREV = 300, 1000   # :2333, :2424
    SC_CAP = 150.0                  # :2431

    def __init__(self, keymap: KeyFrameMap, historyKeyframeSearchRadius: float = 30.0, historyKeyframeSearchTimeDiff: float = 30.0, historyKeyframeSearchNum: int = 25,
                 historyKeyframeFitnessScore: float = 0.3, sc_yaw_guess: float = 0.0):
        """sc_yaw_guess: the SC form's ICP starts from pcl::getTransformation(0, 0, 0, 0, 0, sc_yaw_guess * yawDiffRad). 0 (default) is the reference as written: it
        computes the guess and aligns without it (:2437-2443); +1 is its commented-out line; -1 turns the current scan onto the loop scan when key 0's pose is the
        origin (yawDiffRad is the turn from the loop scan to the current one)."""
        self.km = keymap
        self.sc_yaw_guess = sc_yaw_guess
        self.radius, self.time_diff, self.search_num, self.fitness_score = historyKeyframeSearchRadius, historyKeyframeSearchTimeDiff, historyKeyframeSearchNum, historyKeyframeFitnessScore
        self.loopIndexContainer = {}
        self.last = None   # the last ICP result, also of a rejected loop

    def _align(self, cur, pre, wrt_key, cap, guess=None):
        self.last = None
        n_cur = self.km.loopCloud(0, cur, 0, wrt_key)
        n_pre = self.km.loopCloud(1, pre, self.search_num, wrt_key)
        if n_cur < self.MIN_CUR or n_pre < self.MIN_PREV:
            return None
        self.last = self.km.loopIcp(loop_icp_params(cap), guess)
        if not self.last["converged"] or self.last["fitness"] > self.fitness_score:   # :2354, :2445
            return None
        return self.last

    def performRSLoopClosure(self, time_cur: float):
        if len(self.km.poses) == 0:
            return None
        cur = len(self.km.poses) - 1
        if cur in self.loopIndexContainer:   # :2487-2489
            return None
        pre = self.km.detect_loop_distance(time_cur, self.radius, self.time_diff)
        if pre < 0:
            return None
        res = self._align(cur, pre, None, 2.0 * self.radius)   # :2342
        if res is None:
            return None
        t_wrong = pose6_to_T(self.km.poses[cur])
        t_correct = (res["T"].astype(np.float32) @ t_wrong).astype(np.float64)   # :2377
        self.loopIndexContainer[cur] = pre
        return LoopFactor((cur, pre, t_correct, pose6_to_T(self.km.poses[pre], np.float64), np.float32(res["fitness"])), robust=None)   # :2382-2385

    def performSCLoopClosure(self, sc_manager: "ScanContextManager"):
        if len(self.km.poses) == 0:
            return None
        pre, yaw = sc_manager.detectLoopClosureID()
        cur = len(self.km.poses) - 1
        if pre == -1 or cur == pre:
            return None
        guess = pose6_to_T([0.0, 0.0, np.float32(self.sc_yaw_guess) * np.float32(yaw), 0.0, 0.0, 0.0]) if self.sc_yaw_guess != 0.0 else None
        res = self._align(cur, pre, 0, self.SC_CAP, guess)   # baseKey 0, :2421-2423
        if res is None:
            return None
        self.loopIndexContainer[cur] = pre
        return LoopFactor((cur, pre, res["T"].astype(np.float64), np.eye(4), np.float32(res["fitness"])), robust=1.0)   # :2468-2470



def pgo_params(**kw) -> PgoParams:
    """GTSAM's LevenbergMarquardtParams defaults (rolo_pgo_default_params); fields of rolo_pgo_params by keyword"""
    p = PgoParams()
    lib().rolo_pgo_default_params(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


class PoseGraph:
    """gtSAMgraph + initialEstimate + isam->update + correctPoses (:1094-1320) as a batch minimiser of the same objective on the device (include/rolo_hip.h,
    "pose-graph optimisation"): the same factors and noise models, the SC loop's Cauchy-robust noise included; iSAM2's incremental bookkeeping and its marginal
    covariance are not restated, and parity with GTSAM is unpinned. Poses are 4 x 4 doubles; pose6 is transformTobeMapped order (roll, pitch, yaw, x, y, z)."""
    STATES = ("NONE", "CONVERGED", "ITERATIONS", "LAMBDA")
    PRIOR_VARIANCES = (1e-2, 1e-2, np.pi * np.pi, 1e8, 1e8, 1e8)   # :1229
    ODOM_VARIANCES = (1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4)          # :1235

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(lib().rolo_pgo_create(device, C.byref(self._h)), "rolo_pgo_create")
        self._last = None   # the graph's last pose (4 x 4), kept on the host between optimisations
        self.last = None    # the last optimise's result

    def close(self):
        if self._h:
            lib().rolo_pgo_destroy(self._h)
            self._h = C.c_void_p()

    def size(self):
        """(poses, factors, chords)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().rolo_pgo_size(self._h, C.byref(a), C.byref(b), C.byref(c)), "rolo_pgo_size")
        return a.value, b.value, c.value

    def __len__(self):
        return self.size()[0]

    @staticmethod
    def _dp(a, n):
        a = np.ascontiguousarray(a, np.float64).reshape(n)
        return a, a.ctypes.data_as(C.POINTER(C.c_double))

    def addPose(self, T) -> int:
        keep, p = self._dp(T, 16)
        k = check(lib().rolo_pgo_add_pose(self._h, p), "rolo_pgo_add_pose")
        self._last = keep.reshape(4, 4).copy()
        return k

    def addPrior(self, i: int, T, variances):
        kt, t = self._dp(T, 16); kv, v = self._dp(variances, 6)
        check(lib().rolo_pgo_add_prior(self._h, i, t, v), "rolo_pgo_add_prior")

    def addBetween(self, i: int, j: int, T, variances, cauchy=None):
        """BetweenFactor<Pose3>(i, j, T, Diagonal::Variances(variances)); the reference's ground-prior factors (:1266-1284) come through here. cauchy = k puts the
        noise under Robust::Create(mEstimator::Cauchy::Create(k), ...) as the SC loop closure does (:2464-2470); None is the plain diagonal"""
        kt, t = self._dp(T, 16); kv, v = self._dp(variances, 6)
        if cauchy is None:
            check(lib().rolo_pgo_add_between(self._h, i, j, t, v), "rolo_pgo_add_between")
        else:
            check(lib().rolo_pgo_add_between_robust(self._h, i, j, t, v, PGO_LOSS_CAUCHY, float(cauchy)), "rolo_pgo_add_between_robust")

    def addOdomFactor(self, pose6) -> int:
        """addOdomFactor (:1224-1243): the first call adds the prior, later ones poseFrom.between(poseTo) from the graph's last pose; returns the new pose's index"""
        T = pose6_to_T(pose6, np.float64)
        if self._last is None:
            k = self.addPose(T)
            self.addPrior(k, T, self.PRIOR_VARIANCES)
            return k
        prev = self._last
        k = self.addPose(T)
        self.addBetween(k - 1, k, np.linalg.inv(prev) @ T, self.ODOM_VARIANCES)
        return k

    def addLoopFactor(self, loop):
        """addLoopFactor (:1245-1264) for one (cur, pre, poseFrom, poseTo, noise) of LoopCloser: between(cur, pre, poseFrom^-1 poseTo, noise on all six). A
        LoopFactor whose `robust` is k, as performSCLoopClosure returns it, becomes a factor under Cauchy(k); a plain tuple or robust = None a plain one"""
        cur, pre, pose_from, pose_to, noise = loop
        Z = np.linalg.inv(np.asarray(pose_from, np.float64)) @ np.asarray(pose_to, np.float64)
        self.addBetween(int(cur), int(pre), Z, np.full(6, float(noise)), cauchy=getattr(loop, "robust", None))

    def addPriorFactor(self, f):
        """addPriorFactor (:1266-1284) for one PriorFactor of GroundPriorCloser: between(linked, current, poseFrom^-1 poseTo, its six variances), plain noise"""
        linked, current, pose_from, pose_to, variances = f
        Z = np.linalg.inv(np.asarray(pose_from, np.float64)) @ np.asarray(pose_to, np.float64)
        self.addBetween(int(linked), int(current), Z, np.asarray(variances, np.float64))

    def optimize(self, params: PgoParams = None) -> dict:
        res = PgoResult()
        check(lib().rolo_pgo_optimize(self._h, C.byref(params if params is not None else pgo_params()), C.byref(res)), "rolo_pgo_optimize")
        self.last = dict(state=res.state, iterations=res.iterations, trials=res.trials, initial_cost=res.initial_cost, final_cost=res.final_cost, lambda_=res.lambda_,
                         pcg_iterations=res.pcg_iterations)
        if res.iterations > 0:   # the poses moved: the host's copy of the last one is stale
            n = len(self)
            self._last = self.poses()[n - 1].copy()
        return self.last

    def poses(self):
        """n x 4 x 4 doubles"""
        n = len(self)
        T = np.zeros((max(n, 1), 16), np.float64)
        check(lib().rolo_pgo_get_poses(self._h, T.ctypes.data_as(C.POINTER(C.c_double)), None, n), "rolo_pgo_get_poses")
        return T[:n].reshape(n, 4, 4)

    def poses6(self):
        """n x 6 floats, transformTobeMapped order"""
        n = len(self)
        p = np.zeros((max(n, 1), 6), np.float32)
        check(lib().rolo_pgo_get_poses(self._h, None, p.ctypes.data_as(C.POINTER(C.c_float)), n), "rolo_pgo_get_poses")
        return p[:n]

    def trace(self):
        """one record per trial of the last optimise"""
        n = check(lib().rolo_pgo_get_trace(self._h, None, 0), "rolo_pgo_get_trace")
        recs = (PgoTraceRec * max(n, 1))()
        check(lib().rolo_pgo_get_trace(self._h, recs, n), "rolo_pgo_get_trace")
        return [dict(lambda_=r.lambda_, cost=r.cost, accepted=bool(r.accepted), pcg_iterations=r.pcg_iterations, residual=r.residual) for r in recs[:n]]

    def factorErrors(self):
        """(r2, w): every factor's r^2 = |e / sigma|^2 and weight at the current poses, in the order the factors were added; w is 1.0 for a factor without
        loss, and near 0 for a robust loop that the optimum outvoted"""
        f = self.size()[1]
        r2 = np.zeros(max(f, 1), np.float64); w = np.zeros(max(f, 1), np.float64)
        dp = C.POINTER(C.c_double)
        check(lib().rolo_pgo_get_factor_errors(self._h, r2.ctypes.data_as(dp), w.ctypes.data_as(dp), f), "rolo_pgo_get_factor_errors")
        return r2[:f], w[:f]

    SOLVE_FORMS = ("auto", "one", "grid")   # ROLO_PGO_SOLVE_AUTO, _ONE_WG, _GRID

    def setSolveForm(self, form: str):
        """which form the solves of this graph take: "one" (one workgroup), "grid" (launches that cover the device) or "auto" (the default: by pose count).
        Both forms return the same bits; anything else is an error and the form stays as it was"""
        check(lib().rolo_pgo_set_solve_form(self._h, self.SOLVE_FORMS.index(form) if form in self.SOLVE_FORMS else -1), "rolo_pgo_set_solve_form")

    def solveForm(self):
        """(requested, last_used) as the names of setSolveForm; last_used is None before any solve"""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().rolo_pgo_get_solve_form(self._h, C.byref(a), C.byref(b)), "rolo_pgo_get_solve_form")
        return self.SOLVE_FORMS[a.value], (self.SOLVE_FORMS[b.value] if b.value else None)

    def lastMs(self):
        """device milliseconds of the last optimise: linearise + assemble, factorisation, PCG, retract + cost"""
        ms = np.zeros(4, np.float32)
        check(lib().rolo_pgo_last_ms(self._h, ms.ctypes.data_as(C.POINTER(C.c_float))), "rolo_pgo_last_ms")
        return ms

    def correctPoses(self, keymap: KeyFrameMap):
        """correctPoses (:1287-1320): the graph's poses into the key map (the first len(graph) key frames); the next extraction uses them"""
        keymap.setPoses(self.poses6())

    def linearize(self):
        """test hook -> cost, grad (6N), diag (N x 6 x 6), chain ((N - 1) x 6 x 6), chord (C x 6 x 6), chord_ij (C x 2)"""
        n, _, nc = self.size()
        dp = C.POINTER(C.c_double)
        cost = C.c_double(0.0)
        g = np.zeros(6 * n); D = np.zeros((n, 6, 6)); Ch = np.zeros((max(n - 1, 1), 6, 6)); H = np.zeros((max(nc, 1), 6, 6)); ij = np.zeros((max(nc, 1), 2), np.int32)
        check(lib().rolo_pgo_linearize(self._h, C.byref(cost), g.ctypes.data_as(dp), D.ctypes.data_as(dp), Ch.ctypes.data_as(dp), H.ctypes.data_as(dp),
                                       ij.ctypes.data_as(C.POINTER(C.c_int32))), "rolo_pgo_linearize")
        return cost.value, g, D, Ch[:max(n - 1, 0)], H[:nc], ij[:nc]

    def solveLinear(self, lambda_: float = 0.0, pcg_tol: float = 1e-10, pcg_max: int = 0):
        """test hook -> delta (6N), PCG iterations, sqrt(r z) / sqrt(r0 z0): the step a trial would take on the last linearize()"""
        n = len(self)
        d = np.zeros(6 * max(n, 1)); its = C.c_int(0); res = C.c_double(0.0)
        check(lib().rolo_pgo_solve_linear(self._h, lambda_, pcg_tol, pcg_max, d.ctypes.data_as(C.POINTER(C.c_double)), C.byref(its), C.byref(res)), "rolo_pgo_solve_linear")
        return d[:6 * n], its.value, res.value


def prior_pose_params(wheel_xy=None, square_size=None, **kw) -> PriorPoseParams:
    """config/prior_pose_params.yaml's values; wheel_xy (k x 2, body frame) or square_size (VehicleModel::FromSquare's four corners) replace its wheels; fields of
    rolo_priorpose_params by keyword (body_to_lidar_t: 3, body_to_lidar_R: 3 x 3 row-major)"""
    p = PriorPoseParams()
    lib().rolo_priorpose_default_params(C.byref(p))
    if square_size is not None:
        h = square_size / 2.0
        wheel_xy = [(-h, h), (h, h), (h, -h), (-h, -h)]
    if wheel_xy is not None:
        w = np.asarray(wheel_xy, np.float64).reshape(-1, 2)
        p.n_wheels = w.shape[0]
        for k in range(min(w.shape[0], 8)):   # more than 8: n_wheels says so and the call refuses it
            p.wheel_xy[2 * k], p.wheel_xy[2 * k + 1] = w[k]
    for k, v in kw.items():
        assert hasattr(p, k), k
        if k in ("body_to_lidar_t", "body_to_lidar_R"):
            v = np.asarray(v, np.float64).reshape(-1)
            for i in range(v.shape[0]):
                getattr(p, k)[i] = v[i]
        else:
            setattr(p, k, v)
    return p


class GroundModel:
    """ground_factor::GroundModel (pose_solver.cpp:120-376) resident on the device: the ground cloud (n x stride floats, x y z first, 3 <= stride <= 8), its x-y
    queries and ExtractPatch."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(lib().rolo_ground_create(device, C.byref(self._h)), "rolo_ground_create")

    def close(self):
        if self._h:
            lib().rolo_ground_destroy(self._h)
            self._h = C.c_void_p()

    def setGrid(self, cell_size: float = 0.6, max_cells: int = 1 << 22):
        check(lib().rolo_ground_set_grid(self._h, cell_size, max_cells), "rolo_ground_set_grid")

    def setCloud(self, cloud):
        """UpdateFromCloud. An empty cloud empties the model"""
        a = np.ascontiguousarray(cloud, np.float32)
        a = a.reshape(-1, a.shape[-1] if a.ndim > 1 else 4)
        check(lib().rolo_ground_set_cloud(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], a.shape[1]), "rolo_ground_set_cloud")

    def info(self) -> dict:
        v = (C.c_longlong * 5)()
        check(lib().rolo_ground_info(self._h, v, 5), "rolo_ground_info")
        return dict(points=v[0], nx=v[1], ny=v[2], doubled=v[3], stride=v[4])

    def nearestXY(self, xy):
        """test hook -> (index, d2) per query (n x 2, taken as float)"""
        q = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        idx = np.zeros(q.shape[0], np.int32); d2 = np.zeros(q.shape[0], np.float32)
        check(lib().rolo_ground_nearest_xy(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                           d2.ctypes.data_as(C.POINTER(C.c_float))), "rolo_ground_nearest_xy")
        return idx, d2

    def radiusXY(self, xy, radius: float, cap: int = 4096):
        """test hook -> per query (count, indices, d2) of the sorted radius search; the lists are empty when count exceeds 4096, cut at cap otherwise"""
        q = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        nq = q.shape[0]
        cnt = np.zeros(nq, np.int32); idx = np.zeros((nq, max(cap, 1)), np.int32); d2 = np.zeros((nq, max(cap, 1)), np.float32)
        check(lib().rolo_ground_radius_xy(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), nq, radius, cap, cnt.ctypes.data_as(C.POINTER(C.c_int32)),
                                          idx.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(C.POINTER(C.c_float))), "rolo_ground_radius_xy")
        out = []
        for k in range(nq):
            m = min(int(cnt[k]), cap) if cnt[k] <= 4096 else 0
            out.append((int(cnt[k]), idx[k, :m].copy(), d2[k, :m].copy()))
        return out

    def extractPatch(self, cx: float, cy: float, patch_size: float, T=None):
        """ExtractPatch, then (T given, 4 x 4) pcl::transformPointCloud in float: the kept records in the cloud's order, possibly none"""
        st = self.info()
        n, stride = st["points"], st["stride"]
        out = np.zeros((max(n, 1), max(stride, 3)), np.float32)
        m = C.c_int(0)
        keep, t = _guess_ptr(T)
        check(lib().rolo_ground_extract_patch(self._h, cx, cy, patch_size, t, out.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(m)), "rolo_ground_extract_patch")
        return out[:m.value].copy()

    def lastMs(self):
        """device milliseconds of the last grid build, patch and solve"""
        ms = np.zeros(3, np.float32)
        check(lib().rolo_ground_last_ms(self._h, ms.ctypes.data_as(C.POINTER(C.c_float))), "rolo_ground_last_ms")
        return ms


class PriorPoseSolver:
    """ground_factor::PoseSolver (pose_solver.cpp:379-679) over a resident GroundModel, for whole arrays of poses, and what PriorPoseNode::HandlePose
    (prior_pose_node.cpp:164-233) publishes from one."""
    END_REASONS = ("converged", "max_iters")
    FALLBACKS = ("fit", "few_hits", "few_inliers", "no_plane", "vertical", "overflow")

    def __init__(self, ground: GroundModel, params: PriorPoseParams = None, groundPatchSize: float = 20.0):
        self.ground = ground
        self.params = params if params is not None else prior_pose_params()
        self.patch_size = groundPatchSize

    def solve(self, xyyaw) -> dict:
        """(B x 3) poses -> arrays per field: z, roll, pitch, R (B x 3 x 3), cost, wheel_distance (B x wheels), lidar_pose (B x 6: x y z roll pitch yaw),
        iterations, end_reason, success, status"""
        q = np.ascontiguousarray(xyyaw, np.float64).reshape(-1, 3)
        B = q.shape[0]
        res = (PriorPoseResult * max(B, 1))()
        check(lib().rolo_priorpose_solve(self.ground._h, C.byref(self.params), q.ctypes.data_as(C.POINTER(C.c_double)), B, res), "rolo_priorpose_solve")
        W = self.params.n_wheels
        return dict(z=np.array([r.z for r in res]), roll=np.array([r.roll for r in res]), pitch=np.array([r.pitch for r in res]),
                    R=np.array([list(r.R) for r in res]).reshape(B, 3, 3), cost=np.array([r.cost for r in res]),
                    wheel_distance=np.array([list(r.wheel_distance)[:W] for r in res]), lidar_pose=np.array([list(r.lidar_pose) for r in res]),
                    iterations=np.array([r.iterations for r in res], np.int32), end_reason=np.array([r.end_reason for r in res], np.int32),
                    success=np.array([bool(r.success) for r in res]), status=np.array([r.status for r in res], np.int32))

    def fitSurface(self, xy) -> dict:
        """test hook: FitLocalSurface (or its nearest-point fall-back) at (n x 2) double queries -> hits, inliers, fallback, nearest, point (n x 3)"""
        q = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        res = (PriorPoseFit * max(q.shape[0], 1))()
        check(lib().rolo_priorpose_fit_surface(self.ground._h, C.byref(self.params), q.ctypes.data_as(C.POINTER(C.c_double)), q.shape[0], res), "rolo_priorpose_fit_surface")
        return dict(hits=np.array([r.hits for r in res], np.int32), inliers=np.array([r.inliers for r in res], np.int32),
                    fallback=np.array([r.fallback for r in res], np.int32), nearest=np.array([r.nearest for r in res], np.int32),
                    point=np.array([list(r.point) for r in res]))

    def handlePose(self, x: float, y: float, yaw: float):
        """HandlePose: None unless the solve succeeds; else (initialGuess X Y Z Roll Pitch Yaw as float32, the ground patch around the lidar's x y in the lidar
        pose's frame). The patch's transform is T_world_lidar^-1 inverted in double and cast to float, as the reference casts it."""
        r = self.solve([[x, y, yaw]])
        if not r["success"][0]:
            return None
        lp = r["lidar_pose"][0]
        T = pose6_to_T([lp[3], lp[4], lp[5], lp[0], lp[1], lp[2]], np.float64)
        patch = self.ground.extractPatch(lp[0], lp[1], float(self.patch_size), np.linalg.inv(T).astype(np.float32))
        return lp.astype(np.float32), patch


# ---- the ground prior's association (performPriorAssociation, src/backMapping.cpp:1943-2158) ------------------------------------------------------------------
_f32 = np.float32


def _mul34(a, b):
    """Affine3f a * b in float32: linear = La Lb, translation = La tb + ta (each entry a0 b0 + a1 b1 + a2 b2, left to right)"""
    a, b = np.asarray(a, _f32), np.asarray(b, _f32)
    o = np.eye(4, dtype=_f32)
    for i in range(3):
        for j in range(4):
            x = a[i, 0] * b[0, j]
            x = _f32(x + a[i, 1] * b[1, j])
            x = _f32(x + a[i, 2] * b[2, j])
            o[i, j] = _f32(x + a[i, 3]) if j == 3 else x
    return o


def _inv34(a):
    """Affine3f::inverse() in float32: the 3 x 3 inverse by cofactors over the determinant (Eigen's compute_inverse<3>), translation = -(L^-1 t)"""
    a = np.asarray(a, _f32)
    m = a[:3, :3]
    cof = lambda i, j: _f32(m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3] - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3])
    c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]   # the first column of the inverse, before the division
    det = _f32(_f32(m[0, 0] * c0[0] + m[1, 0] * c0[1]) + m[2, 0] * c0[2])
    inv = _f32(1.0) / det
    o = np.eye(4, dtype=_f32)
    for i in range(3):
        for j in range(3):
            o[i, j] = cof(j, i) * inv
    for i in range(3):
        o[i, 3] = -_f32(_f32(o[i, 0] * a[0, 3] + o[i, 1] * a[1, 3]) + o[i, 2] * a[2, 3])
    return o


def _euler34(T):
    """pcl::getTranslationAndEulerAngles in float32 -> (x, y, z, roll, pitch, yaw)"""
    T = np.asarray(T, _f32)
    return T[0, 3], T[1, 3], T[2, 3], np.arctan2(T[2, 1], T[2, 2]), np.arcsin(-T[2, 0]), np.arctan2(T[1, 0], T[0, 0])


def _quat_from_R(m):
    """Eigen::Quaternionf(Matrix3f) in float32 -> (w, x, y, z)"""
    m = np.asarray(m, _f32)
    t = _f32(_f32(m[0, 0] + m[1, 1]) + m[2, 2])
    q = np.zeros(4, _f32)
    if t > 0:
        t = np.sqrt(_f32(t + _f32(1.0)))
        q[0] = _f32(0.5) * t
        t = _f32(0.5) / t
        q[1], q[2], q[3] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(_f32(_f32(_f32(m[i, i] - m[j, j]) - m[k, k]) + _f32(1.0)))
        q[1 + i] = _f32(0.5) * t
        t = _f32(0.5) / t
        q[0] = (m[k, j] - m[j, k]) * t
        q[1 + j] = (m[j, i] + m[i, j]) * t
        q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def _quat_norm(q):
    n = np.sqrt(_f32(_f32(_f32(q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
    return (q / n).astype(_f32)


def _quat_mul(a, b):
    """Hamilton product in float32, (w, x, y, z)"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx], _f32)


def _quat_axis(angle, axis):
    """Quaternionf(AngleAxisf(angle, unit axis `axis`))"""
    h = _f32(0.5) * _f32(angle)
    q = np.zeros(4, _f32)
    q[0], q[1 + axis] = np.cos(h), np.sin(h)
    return q


def _quat_slerp(a, t, b):
    """Eigen's QuaternionBase::slerp in float32: the linear branch at |a . b| >= 1 - epsilon, the second weight negated for a negative dot"""
    t = _f32(t)
    d = _f32(_f32(_f32(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3])
    ad = np.abs(d)
    if ad >= _f32(1.0) - np.finfo(_f32).eps:
        s0, s1 = _f32(1.0) - t, t
    else:
        th = np.arccos(ad)
        st = np.sin(th)
        s0, s1 = np.sin(_f32(_f32(1.0) - t) * th) / st, np.sin(t * th) / st
    if d < 0:
        s1 = -s1
    return (_f32(s0) * a + _f32(s1) * b).astype(_f32)


def _quat_to_R(q):
    """Quaternionf::toRotationMatrix in float32"""
    w, x, y, z = (_f32(v) for v in q)
    tx, ty, tz = _f32(2.0) * x, _f32(2.0) * y, _f32(2.0) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = _f32(1.0)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]], _f32)


def _wrap_abs(a):
    """|atan2(sin a, cos a)| in float32 (:2089-2090)"""
    a = _f32(a)
    return np.abs(np.arctan2(np.sin(a), np.cos(a)))


PRIOR_WEIGHT = 0.2   # priorWeight, :2067


def prior_association_gates(linked_key_pose, current_key_pose, relative_prior_pose, T, fitness, priorRotDiffTolerance, priorTransDiffTolerance=1.0,
                            priorFactorWeight=100.0):
    """performPriorAssociation from the accepted ICP to the factor (:2054-2125) in float32, host only. The three poses and the ICP's T are 4 x 4 (Affine3f);
    priorRotDiffTolerance is in RADIANS here (the reference converts its parameter on loading, utility.h:368; GroundPriorCloser takes degrees as the parameter file
    does). Returns a dict: `rejected` is None, "z", "roll" or "pitch" (the first failing gate in the reference's order of tests); `diff` = (diff_z, diff_roll,
    diff_pitch); `odom` / `prior` = (dx, dy, dz, roll, pitch, yaw) of tbbPrevToCur / tbbPrevToCur_prior; and, when nothing rejected, priorTrans (4 x 4 float32),
    poseFrom, poseTo (4 x 4 float64: RzRyRx of the float Euler angles, as gtsam builds them) and variances (6 float64: s, s, 1e-6f, 1e-6f, 1e-6f, s).
    Where Eigen takes a Transform's rotation() through an SVD (Affine mode), this takes linear(): the poses are rigid up to float rounding."""
    linked, current, relative = (np.asarray(x, _f32).reshape(4, 4) for x in (linked_key_pose, current_key_pose, relative_prior_pose))
    Tf = np.asarray(T, np.float64).reshape(4, 4).astype(_f32)   # getFinalTransformation().cast<double>().cast<float>()
    prev_to_cur = _mul34(current, _inv34(linked))               # :2064
    prev_to_cur_prior = _mul34(Tf, relative)                    # :2065
    odom_q = _quat_norm(_quat_from_R(prev_to_cur[:3, :3]))
    odom = _euler34(prev_to_cur)
    prior = _euler34(prev_to_cur_prior)
    diff_z = np.abs(_f32(odom[2] - prior[2]))
    diff_roll = _wrap_abs(odom[3] - prior[3])
    diff_pitch = _wrap_abs(odom[4] - prior[4])
    out = dict(rejected=None, diff=(diff_z, diff_roll, diff_pitch), odom=odom, prior=prior)
    rot_tol, trans_tol = _f32(priorRotDiffTolerance), _f32(priorTransDiffTolerance)
    if diff_z > trans_tol:
        out["rejected"] = "z"
    elif diff_roll > rot_tol:
        out["rejected"] = "roll"
    elif diff_pitch > rot_tol:
        out["rejected"] = "pitch"
    if out["rejected"] is not None:
        return out
    target_q = _quat_norm(_quat_mul(_quat_mul(_quat_axis(odom[5], 2), _quat_axis(prior[4], 1)), _quat_axis(prior[3], 0)))   # Rz(odom yaw) Ry(prior pitch) Rx(prior roll)
    blended_q = _quat_norm(_quat_slerp(odom_q, PRIOR_WEIGHT, target_q))
    prior_trans = np.eye(4, dtype=_f32)
    prior_trans[:3, :3] = _quat_to_R(blended_q)
    prior_trans[:3, 3] = prev_to_cur[:3, 3]   # the odometry's translation: the z blend is commented out (:2071)
    x, y, z, r, p, yw = _euler34(linked)
    pose_from = pose6_to_T([float(r), float(p), float(yw), float(x), float(y), float(z)], np.float64)
    x, y, z, r, p, yw = _euler34(_mul34(prior_trans, linked))   # :2117
    pose_to = pose6_to_T([float(r), float(p), float(yw), float(x), float(y), float(z)], np.float64)
    s = max(_f32(fitness), _f32(1e-6)) * _f32(priorFactorWeight)
    small = np.float64(_f32(1e-6))
    out.update(priorTrans=prior_trans, poseFrom=pose_from, poseTo=pose_to, variances=np.array([s, s, small, small, small, s], np.float64))
    return out


class PriorFactor(tuple):
    """(linked_key, current_key, poseFrom 4 x 4, poseTo 4 x 4, variances6) as GroundPriorCloser returns it: the constraint is poseFrom.between(poseTo) from the
    linked key pose to the current one. PoseGraph.addPriorFactor takes it as it is."""
    def __new__(cls, linked_key, current_key, poseFrom, poseTo, variances6):
        return super().__new__(cls, (linked_key, current_key, poseFrom, poseTo, variances6))

    linked_key = property(lambda self: self[0])
    current_key = property(lambda self: self[1])
    poseFrom = property(lambda self: self[2])
    poseTo = property(lambda self: self[3])
    variances = property(lambda self: self[4])


class GroundPriorCloser:
    """priorInfoHandler (:459-513) and performPriorAssociation (:1943-2158) over a key map's poses: the history of (prior pose, ground patch) entries, the
    candidates near the last key pose, their ICPs against the laser's ground cloud, `batch` at a time through LoopIcp.alignBatch, the gates and the factor.
    The history is never pruned, as in the reference (priorFilter is commented out there). Not here: the ROS thread and its rate, visualizePrior, priorFilter."""

    def __init__(self, keymap, icp: LoopIcp = None, groundPatchSize: float = 2.0, nearPriorRadius: float = 1.0, priorFitnessScore: float = 0.01,
                 priorRotDiffTolerance: float = 5.0, priorTransDiffTolerance: float = 1.0, priorFactorWeight: float = 100.0, priorSyncedInterval: float = 0.0,
                 batch: int = 8):
        """priorRotDiffTolerance in degrees, as the parameter file has it. keymap: anything with `poses` (pose6 per key frame) and `times`; icp: a LoopIcp
        (made on first use when None). batch: candidates per alignBatch call; 1 runs them one launch set each. The default of 8 is from profiles/r18/priorassoc.json: a
        chunk of eight costs about what two to three ICPs cost one after another; raise it where long runs of rejections are the rule."""
        assert 1 <= batch <= LoopIcp.MAX_BATCH
        self.km, self.icp, self._own_icp = keymap, icp, False
        self.patch_size, self.radius, self.fitness_score = _f32(groundPatchSize), _f32(nearPriorRadius), _f32(priorFitnessScore)
        self.rot_tol = _f32(_f32(priorRotDiffTolerance) * np.pi / _f32(180.0))   # utility.h:368 (float * double / float -> float)
        self.trans_tol, self.weight, self.synced_interval = _f32(priorTransDiffTolerance), _f32(priorFactorWeight), _f32(priorSyncedInterval)
        self.batch = int(batch)
        self.priorPosePatchHistory, self.priorTimeKeyQueue = [], []
        self.ground_cloud = np.zeros((0, 4), np.float32)
        self.priorVisContainer = {}
        # per candidate the last performPriorAssociation aligned, in history order: dict(entry, linked_key, icp, rejected, gates); rejected is None (the factor's),
        # "fitness", "z", "roll", "pitch", or "unused" for what shared the accepted candidate's chunk behind it and was never judged
        self.last = []

    def close(self):
        if self._own_icp and self.icp is not None:
            self.icp.close()
            self.icp = None

    def priorInfoHandler(self, msg_time: float, prior_pose6, patch) -> bool:
        """prior_pose6: initialGuess roll, pitch, yaw, x, y, z. True when the entry was stored"""
        if len(self.km.poses) == 0:
            return False
        latest_time, latest_id = self.km.times[-1], len(self.km.poses) - 1
        if latest_id <= 9 or abs(float(msg_time) - latest_time) >= 1e-2:
            return False
        if self.priorTimeKeyQueue and self.synced_interval > 0.0:
            if float(msg_time) - self.priorTimeKeyQueue[-1][0] < float(self.synced_interval):
                return False
        pose = np.asarray(prior_pose6, np.float32).reshape(6).astype(np.float64)   # priorPoseCur is float[6]
        self.priorPosePatchHistory.append((pose, np.ascontiguousarray(patch, np.float32).reshape(-1, 4).copy()))
        self.priorTimeKeyQueue.append((float(msg_time), latest_id))
        return True

    def setGroundCloud(self, patch):
        """GroundCloudFromlaser (groundMapHandler): the ICPs' target, e.g. GroundModel.extractPatch(0, 0, groundPatchSize)"""
        self.ground_cloud = np.ascontiguousarray(patch, np.float32).reshape(-1, 4).copy()

    def candidates(self):
        """the history entries the reference would run an ICP for, in order: (entry index, linked key, linked pose, relative prior pose), all float32 4 x 4"""
        out = []
        if len(self.km.poses) == 0:
            return out
        current = pose6_to_T(self.km.poses[-1])
        for e, ((pose, patch), (_, linked_id)) in enumerate(zip(self.priorPosePatchHistory, self.priorTimeKeyQueue)):
            linked = pose6_to_T(self.km.poses[linked_id])
            relative = pose6_to_T(pose.astype(np.float32))   # pcl::getTransformation takes floats
            g = _mul34(linked, relative)
            dx, dy = _f32(g[0, 3] - current[0, 3]), _f32(g[1, 3] - current[1, 3])
            dist = float(np.sqrt(_f32(dx * dx + dy * dy)))
            if dist < float(self.radius) and patch.shape[0] > 0 and self.ground_cloud.shape[0] > 0:
                out.append((e, linked_id, linked, relative))
        return out

    def performPriorAssociation(self):
        self.last = []
        if len(self.km.poses) == 0 or not self.priorPosePatchHistory:
            return None
        if self.icp is None:
            self.icp, self._own_icp = LoopIcp(), True
        current_id = len(self.km.poses) - 1
        current = pose6_to_T(self.km.poses[-1])
        cands = self.candidates()
        params = loop_icp_params(float(self.patch_size), max_iterations=100, transformation_epsilon=1e-6, euclidean_fitness_epsilon=1e-6)
        for c0 in range(0, len(cands), self.batch):
            chunk = cands[c0:c0 + self.batch]
            results = self.icp.alignBatch([self.priorPosePatchHistory[e][1] for e, _, _, _ in chunk], self.ground_cloud, params)
            for k, ((e, linked_id, linked, relative), res) in enumerate(zip(chunk, results)):
                rec = dict(entry=e, linked_key=linked_id, icp=res, rejected=None, gates=None)
                self.last.append(rec)
                if not res["converged"] or res["fitness"] > float(self.fitness_score):   # :2048
                    rec["rejected"] = "fitness"
                    continue
                g = prior_association_gates(linked, current, relative, res["T"], res["fitness"], self.rot_tol, self.trans_tol, self.weight)
                rec["gates"], rec["rejected"] = g, g["rejected"]
                if g["rejected"] is not None:
                    continue
                self.priorVisContainer[current_id] = (linked_id, self.priorPosePatchHistory[e][0].astype(np.float32))   # :2142
                # "Matching only one prior at a time" (:2145): what the chunk aligned behind it is never judged
                self.last += [dict(entry=e2, linked_key=l2, icp=r2, rejected="unused", gates=None) for (e2, l2, _, _), r2 in zip(chunk[k + 1:], results[k + 1:])]
                return PriorFactor(linked_id, current_id, g["poseFrom"], g["poseTo"], g["variances"])
        return None


def mapper_params(**kw) -> MapperParams:
    """utility.h:320-343's defaults (rolo_mapper_default_params); fields of rolo_mapper_params by keyword. sc_input: 0 none, 1 scan_feat, 2 scan_raw"""
    p = MapperParams()
    lib().rolo_mapper_default_params(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


class _BorrowedKeyFrameMap(KeyFrameMap):
    """a mapper's key map under KeyFrameMap's calls: the handle is the mapper's, close() leaves it alone, and the key poses and stamps are read from the library"""

    def __init__(self, owner: "MapOptimization"):
        self._owner = owner
        self._h = C.c_void_p(lib().rolo_mapper_keymap(owner._h))
        self.corner_leaf, self.surf_leaf = owner.params.mappingCornerLeafSize, owner.params.mappingSurfLeafSize
        self.m_corner = self.m_surf = self.m_global = 0

    def close(self):
        pass

    poses = property(lambda self: list(self._owner.keyPoses()[0]))
    times = property(lambda self: list(self._owner.keyPoses()[1]))
    _sizes = property(lambda self: self._owner._sizes)


class _BorrowedPoseGraph(PoseGraph):
    """a mapper's graph under PoseGraph's calls; close() leaves it alone. addOdomFactor belongs to the mapper's scans and is not offered"""

    def __init__(self, owner: "MapOptimization"):
        self._h = C.c_void_p(lib().rolo_mapper_pgo(owner._h))
        self._last = None
        self.last = None

    def close(self):
        pass

    def addOdomFactor(self, pose6):
        raise RuntimeError("a mapper adds its own odometry factors: call MapOptimization.scan")


class MapOptimization:
    """mapOptimization::laserCloudInfoHandler (:420-457) as one call per CloudInfoStamp over rolo_mapper_*: the key map, the scan-to-submap context and the pose
    graph belong to the mapper; `keymap` and `graph` lend them to LoopCloser, ScanContextManager, GroundPriorCloser and the exports between scans."""

    def __init__(self, device: int = 0, params: MapperParams = None, **kw):
        self.params = params if params is not None else mapper_params(**kw)
        self.device = device
        self._h = C.c_void_p()
        check(lib().rolo_mapper_create(device, C.byref(self.params), C.byref(self._h)), "rolo_mapper_create")
        self._sizes = []
        self._keymap = self._graph = None
        self.last = None

    def close(self):
        if self._h:
            lib().rolo_mapper_destroy(self._h)
            self._h = C.c_void_p()

    @property
    def keymap(self) -> KeyFrameMap:
        if self._keymap is None:
            self._keymap = _BorrowedKeyFrameMap(self)
        return self._keymap

    @property
    def graph(self) -> PoseGraph:
        if self._graph is None:
            self._graph = _BorrowedPoseGraph(self)
        return self._graph

    @staticmethod
    def _cloud(x):
        """(keep-alive, address, points, on device) of an n x 4 float32 cloud: a numpy array, or a torch tensor on the mapper's device"""
        if x is None:
            return None, None, 0, None
        if hasattr(x, "data_ptr"):   # torch
            import torch
            t = x.reshape(-1, 4).contiguous()
            assert t.dtype == torch.float32
            if t.is_cuda:
                return t, t.data_ptr() if t.shape[0] else None, t.shape[0], True
            x = t.numpy()
        a = np.ascontiguousarray(x, np.float32).reshape(-1, 4)
        return a, a.ctypes.data if a.shape[0] else None, a.shape[0], False

    def scan(self, stamp: float, corner, surf, raw=None, initialGuess=None) -> dict:
        """one CloudInfoStamp: corner = extracted_corner, surf = extracted_surface ++ extracted_normal, raw = cloud_projected (optional), initialGuess =
        (roll, pitch, yaw, x, y, z) when odomAvailable. All clouds numpy, or all torch tensors on the device (handed over without a copy through the host)."""
        cl = [self._cloud(x) for x in (corner, surf, raw)]
        where = {c[3] for c in cl if c[2]}
        assert len(where) <= 1, "host and device clouds in one scan"
        on_device = bool(where and where.pop())
        if on_device:
            import torch
            torch.cuda.synchronize(self.device)   # the clouds' writers
        g = None if initialGuess is None else np.ascontiguousarray(initialGuess, np.float32).reshape(6)
        res = MapperResult()
        check(lib().rolo_mapper_scan(self._h, float(stamp), cl[0][1], cl[0][2], cl[1][1], cl[1][2], cl[2][1], cl[2][2], 1 if on_device else 0,
                                     None if g is None else g.ctypes.data_as(C.POINTER(C.c_float)), 0 if g is None else 1, C.byref(res)), "rolo_mapper_scan")
        if res.keyframe >= 0:
            self._sizes.append(res.n_corner_ds + res.n_surf_ds)
        if res.s2m_ran:   # the borrowed key map's submap() sizes its arrays by these
            self.keymap.m_corner, self.keymap.m_surf = res.m_corner, res.m_surf
        s = res.s2m
        self.last = dict(processed=bool(res.processed), transformTobeMapped=np.array(res.transformTobeMapped, np.float32), incremental6=np.array(res.incremental6, np.float32),
                         s2m_ran=bool(res.s2m_ran), s2m=(s.skipped, s.iterations, s.converged, s.degenerate, s.n_selected), n_corner_ds=res.n_corner_ds,
                         n_surf_ds=res.n_surf_ds, m_corner=res.m_corner, m_surf=res.m_surf, n_listed=res.n_listed, submap_rebuilt=bool(res.submap_rebuilt),
                         keyframe=res.keyframe, loops_added=res.loops_added, priors_added=res.priors_added, poses_corrected=bool(res.poses_corrected),
                         sc_index=res.sc_index, pgo=dict(state=res.pgo.state, iterations=res.pgo.iterations, trials=res.pgo.trials, initial_cost=res.pgo.initial_cost,
                                                         final_cost=res.pgo.final_cost, lambda_=res.pgo.lambda_, pcg_iterations=res.pgo.pcg_iterations))
        return self.last

    @staticmethod
    def _between(f):
        Z = np.linalg.inv(np.asarray(f[2], np.float64)) @ np.asarray(f[3], np.float64)
        return np.ascontiguousarray(Z, np.float64).reshape(16)

    def queueLoop(self, loop):
        """loopIndexQueue &c .push_back for a LoopFactor of LoopCloser: between(cur, pre, poseFrom^-1 poseTo, noise on all six), under Cauchy(robust) when it has one"""
        cur, pre, _, _, noise = loop
        Z = self._between(loop)
        v = np.full(6, float(noise), np.float64)
        k = getattr(loop, "robust", None)
        dp = C.POINTER(C.c_double)
        check(lib().rolo_mapper_queue_loop(self._h, int(cur), int(pre), Z.ctypes.data_as(dp), v.ctypes.data_as(dp), 0.0 if k is None else float(k)), "rolo_mapper_queue_loop")

    def queueLoopBetween(self, i: int, j: int, T, variances, cauchy=None):
        """the same from the measurement itself (4 x 4) and its six variances"""
        Z = np.ascontiguousarray(T, np.float64).reshape(16); v = np.ascontiguousarray(variances, np.float64).reshape(6)
        dp = C.POINTER(C.c_double)
        check(lib().rolo_mapper_queue_loop(self._h, i, j, Z.ctypes.data_as(dp), v.ctypes.data_as(dp), 0.0 if cauchy is None else float(cauchy)), "rolo_mapper_queue_loop")

    def queuePrior(self, f):
        """priorIndexQueue &c .push_back for a PriorFactor of GroundPriorCloser"""
        Z = self._between(f)
        v = np.ascontiguousarray(f[4], np.float64).reshape(6)
        dp = C.POINTER(C.c_double)
        check(lib().rolo_mapper_queue_prior(self._h, int(f[0]), int(f[1]), Z.ctypes.data_as(dp), v.ctypes.data_as(dp)), "rolo_mapper_queue_prior")

    def keyPoses(self):
        """(n x 6 float32 key poses in transformTobeMapped order, n stamps): cloudKeyPoses6D"""
        n = check(lib().rolo_mapper_get_keyposes(self._h, None, None, 0), "rolo_mapper_get_keyposes")
        p = np.zeros((max(n, 1), 6), np.float32); t = np.zeros(max(n, 1), np.float64)
        check(lib().rolo_mapper_get_keyposes(self._h, p.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_double)), n), "rolo_mapper_get_keyposes")
        return p[:n], t[:n]

    def lastScan(self):
        """laserCloudCornerLastDS, laserCloudSurfLastDS of the last processed scan"""
        fp = C.POINTER(C.c_float)
        cnt = (C.c_int * 2)()
        check(lib().rolo_mapper_get_scan(self._h, None, 0, None, 0, cnt), "rolo_mapper_get_scan")
        c = np.zeros((cnt[0], 4), np.float32); s = np.zeros((cnt[1], 4), np.float32)
        check(lib().rolo_mapper_get_scan(self._h, c.ctypes.data_as(fp), cnt[0], s.ctypes.data_as(fp), cnt[1], None), "rolo_mapper_get_scan")
        return c, s

    def registered(self):
        """publishFrames :1405-1414: the last scan's two filtered clouds at transformTobeMapped, corners first"""
        cnt = (C.c_int * 2)()
        check(lib().rolo_mapper_get_scan(self._h, None, 0, None, 0, cnt), "rolo_mapper_get_scan")
        out = np.zeros((cnt[0] + cnt[1], 4), np.float32)
        n = check(lib().rolo_mapper_get_registered(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.shape[0]), "rolo_mapper_get_registered")
        return out[:n]

    def registeredRaw(self, n_raw: int):
        """:1416-1424: the last scan's raw cloud (n_raw points, as handed to scan) at transformTobeMapped"""
        out = np.zeros((n_raw, 4), np.float32)
        n = check(lib().rolo_mapper_get_registered_raw(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n_raw), "rolo_mapper_get_registered_raw")
        return out[:n]

    def lastMs(self):
        """device milliseconds of the last processed scan: down-sample, sub-map, scan2map, key-frame commit, graph, whole call"""
        ms = np.zeros(6, np.float32)
        check(lib().rolo_mapper_last_ms(self._h, ms.ctypes.data_as(C.POINTER(C.c_float))), "rolo_mapper_last_ms")
        return ms


def mapper_initial_guess(tf6, have_keyposes: bool, guess6, last_odom12, last_odom_available: bool):
    """updateInitialGuess (:516-555) -> (tf6, lastOdom12, lastOdomAvailable); guess6 None: odomAvailable false. Host only."""
    fp = C.POINTER(C.c_float)
    tf = np.ascontiguousarray(tf6, np.float32).reshape(6); out = np.zeros(6, np.float32)
    lo = np.ascontiguousarray(last_odom12, np.float32).reshape(12).copy()
    g = None if guess6 is None else np.ascontiguousarray(guess6, np.float32).reshape(6)
    flag = C.c_int(1 if last_odom_available else 0)
    check(lib().rolo_mapper_initial_guess(tf.ctypes.data_as(fp), 1 if have_keyposes else 0, None if g is None else g.ctypes.data_as(fp), 0 if g is None else 1,
                                          lo.ctypes.data_as(fp), C.byref(flag), out.ctypes.data_as(fp)), "rolo_mapper_initial_guess")
    return out, lo, bool(flag.value)


def mapper_save_frame(last_keypose6, tf6, dist_thr: float = 1.0, angle_thr: float = 0.2) -> bool:
    """saveFrame (:1071-1091); last_keypose6 None: no key frame yet. Host only."""
    fp = C.POINTER(C.c_float)
    a = None if last_keypose6 is None else np.ascontiguousarray(last_keypose6, np.float32).reshape(6)
    b = np.ascontiguousarray(tf6, np.float32).reshape(6)
    return check(lib().rolo_mapper_save_frame(None if a is None else a.ctypes.data_as(fp), b.ctypes.data_as(fp), dist_thr, angle_thr), "rolo_mapper_save_frame") == 1


def mapper_incremental(front6, back6, tf6, started: bool, incre12):
    """publishOdometry's incremental pose (:1361-1389) -> (incre12, x y z roll pitch yaw). Host only."""
    fp = C.POINTER(C.c_float)
    a = [np.ascontiguousarray(x, np.float32).reshape(6) for x in (front6, back6, tf6)]
    inc = np.ascontiguousarray(incre12, np.float32).reshape(12).copy(); out = np.zeros(6, np.float32)
    check(lib().rolo_mapper_incremental(a[0].ctypes.data_as(fp), a[1].ctypes.data_as(fp), a[2].ctypes.data_as(fp), 1 if started else 0, inc.ctypes.data_as(fp),
                                        out.ctypes.data_as(fp)), "rolo_mapper_incremental")
    return inc, out
