"""A NumPy model of the resident keyframe map's append rule (pr_map_append_dev): the seven buffers, the state, the flags,
dropped rows and info - written from the rule's text, not from the kernels."""
import numpy as np

OVERFLOW, DROPPED = 1, 2


class MapModel:
    def __init__(self, keyframe_capacity, point_capacity, max_cloud_points, max_append=1):
        self.kcap, self.pcap, self.max_cloud, self.max_append = keyframe_capacity, point_capacity, max_cloud_points, max_append
        self.xyz = np.zeros((point_capacity, 3), np.float64)
        self.inten = np.zeros(point_capacity, np.float32)
        self.poses = np.zeros((keyframe_capacity, 12), np.float64)
        self.ids = np.zeros(keyframe_capacity, np.int32)
        self.reset()

    def reset(self):
        """offs, frames and state to zero; the other buffers keep their bytes"""
        self.offs = np.zeros(self.kcap + 1, np.int64)
        self.frames = np.zeros((self.kcap, 16), np.float64)
        self.state = np.zeros(4, np.int32)

    @property
    def keyframes(self):
        return int(self.state[0])

    def append(self, xyz, inten, offs, frames, poses=None, ids=None, emitted=None, max_points=None):
        """One call; returns info int32 [4] = clouds appended, first row | -1, keyframes after, flags."""
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3); inten = np.asarray(inten, np.float32).reshape(-1)
        offs = np.asarray(offs, np.int64).reshape(-1); N = len(offs) - 1
        frames = np.asarray(frames, np.float64).reshape(N, 16)
        assert 0 <= N <= self.max_append
        max_points = len(xyz) if max_points is None else max_points
        max_points = min(max_points, self.max_cloud * N)
        flags = int(self.state[1])
        if emitted is not None and int(np.asarray(emitted).reshape(-1)[0]) == 0:
            return np.array([0, -1, self.keyframes, flags], np.int32)
        appended, first, seen = 0, -1, 0               # seen: points of the call in front of this cloud
        for i in range(N):
            size = max(int(offs[i + 1] - offs[i]), 0)
            row = self.keyframes
            if row == self.kcap:
                flags |= OVERFLOW
            else:
                fill = int(self.offs[row])
                if size > self.max_cloud or fill + size > self.pcap or (size > 0 and seen + size > max_points):
                    flags |= OVERFLOW | DROPPED
                    self.frames[row] = 0.0
                    self.offs[row + 1] = fill
                else:
                    s = int(offs[i])
                    self.xyz[fill:fill + size] = xyz[s:s + size]
                    self.inten[fill:fill + size] = inten[s:s + size]
                    self.frames[row] = frames[i]
                    self.offs[row + 1] = fill + size
                self.poses[row] = 0.0 if poses is None else np.asarray(poses, np.float64).reshape(N, 12)[i]
                self.ids[row] = -1 if ids is None else np.asarray(ids, np.int32).reshape(N)[i]
                self.state[0] = row + 1
                first = row if first < 0 else first
                appended += 1
            seen += size
        self.state[1] = flags & OVERFLOW               # DROPPED is the call's, OVERFLOW stays until reset
        return np.array([appended, first, self.keyframes, flags], np.int32)

    def arrays(self):
        return dict(xyz=self.xyz, inten=self.inten, offs=self.offs, frames=self.frames, poses=self.poses, ids=self.ids, state=self.state)
