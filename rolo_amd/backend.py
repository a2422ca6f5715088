"""Host mirrors of the back end: the scan-to-submap optimisation (reference src/backMapping.cpp:681-1058) over rolo_scan2map_optimize and the
device-resident key frames with sub-map assembly (:558-678) over rolo_keymap_*."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib, check, Scan2MapStats
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
