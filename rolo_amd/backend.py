"""Host mirrors of the back end: the scan-to-submap optimisation (reference src/backMapping.cpp:681-1058) over rolo_scan2map_optimize, the
device-resident key frames with sub-map assembly (:558-678) over rolo_keymap_* and Scan Context loop detection (src/scancontext/Scancontext.cpp) over
rolo_keymap_sc_*."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, check, Scan2MapStats, ScParams, ScResult
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


class KeyFrameMap:
    """cornerCloudKeyFrames / surfCloudKeyFrames / cloudKeyPoses6D on the device, with extractSurroundingKeyFrames and downsampleCurrentScan"""

    def __init__(self, device: int = 0, mappingCornerLeafSize: float = 0.2, mappingSurfLeafSize: float = 0.4):
        self._h = C.c_void_p()
        check(lib().rolo_keymap_create(device, C.byref(self._h)), "rolo_keymap_create")
        self.corner_leaf, self.surf_leaf = mappingCornerLeafSize, mappingSurfLeafSize
        self.poses, self.times = [], []   # transformTobeMapped order: roll, pitch, yaw, x, y, z
        self.m_corner = self.m_surf = 0

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
        self.poses.append(p.copy()); self.times.append(float(time))
        return k

    def setPose(self, index: int, pose6):
        """correctPoses (:1301-1314)"""
        p = np.ascontiguousarray(pose6, np.float32).reshape(6)
        check(lib().rolo_keymap_set_pose(self._h, index, p.ctypes.data_as(C.POINTER(C.c_float))), "rolo_keymap_set_pose")
        self.poses[index] = p.copy()

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
