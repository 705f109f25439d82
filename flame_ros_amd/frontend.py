"""Host-side mirror of the feature front end's C ABI (include/flame_hip.h, flame_hip_frontend_*).

`GpuFrontEnd` owns one handle: pose-frame images and feature slots live on the GPU; `track()` takes a grey
image and a world pose and returns the frame's emitted features.  Everything computes in libflame_hip.so;
there is no CPU path in this module (the NumPy restatement the tests compare with is tests/frontend_ref.py).
"""
import ctypes as C

import numpy as np

from . import lib as _l
from .lib import FlameHipError  # noqa: F401

FE_OK, FE_NO_PARALLAX, FE_OUTSIDE, FE_BAD_MATCH, FE_AMBIGUOUS, FE_NEW, FE_DIED, FE_FREE = 0, 1, 2, 3, 4, 5, 6, -1
REF_GRAD = FE_REF_GRAD = 7  # FLAME_HIP_FE_REF_GRAD: refused by the reference-patch gradient gate (set_ref_grad); info key "fail_ref_grad"
COST_SSD, COST_ZSSD = 0, 1  # FLAME_HIP_FE_COST_*: the matching cost (set_cost)
STATUS_KEYS = ("ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died")
IMG_DETECTIONS, IMG_MATCHES = _l.FE_IMG_DETECTIONS, _l.FE_IMG_MATCHES  # FLAME_HIP_FE_IMG_*
PIX_CHANNELS = {_l.PIX_GRAY8: 1, _l.PIX_BGR8: 3, _l.PIX_RGB8: 3, _l.PIX_BGRA8: 4, _l.PIX_RGBA8: 4}


class FrontEndParams(C.Structure):
    """flame_hip_frontend_params."""
    _fields_ = [("detection_win_size", C.c_int32), ("min_grad_mag", C.c_float), ("win_size", C.c_int32),
                ("epipolar_line_var", C.c_float), ("max_dropouts", C.c_int32), ("idepth_min", C.c_float),
                ("idepth_max", C.c_float), ("idepth_init", C.c_float), ("var_init", C.c_float),
                ("max_match_error", C.c_float)]


class Camera(C.Structure):
    """flame_hip_camera."""
    _fields_ = [("raw_width", C.c_int32), ("raw_height", C.c_int32), ("format", C.c_int32), ("resize_factor", C.c_int32),
                ("D", C.c_float * 5)]


class Gates(C.Structure):
    """flame_hip_frontend_gates."""
    _fields_ = [("letterbox", C.c_int32), ("height_gate", C.c_int32), ("min_height", C.c_float), ("max_height", C.c_float),
                ("up", C.c_float * 3)]


def default_frontend_params(**overrides):
    """The library's defaults (flame::Params' feature fields + the front end's own), with overrides."""
    p = FrontEndParams()
    _l.load().flame_hip_frontend_default_params(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(FrontEndParams._fields_):
            raise TypeError("unknown front-end parameter %r" % k)
        setattr(p, k, v)
    return p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pose(T):
    T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1)[:12])
    if T.shape != (12,):
        raise ValueError("a pose is a row-major 3x4 [R|t]")
    return T


class GpuFrontEnd:
    """One `flame_hip_frontend` handle."""

    def __init__(self, width, height, K, max_features=2048, max_poseframes=8, device=0):
        self._lib = _l.load()
        self._h = C.c_void_p()
        self.W, self.H, self.max_features = int(width), int(height), int(max_features)
        K = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        _l.check(self._lib.flame_hip_frontend_create(C.byref(self._h), device, self.W, self.H, _ptr(K), self.max_features,
                                                     int(max_poseframes)), "flame_hip_frontend_create")

    def close(self):
        if self._h:
            self._lib.flame_hip_frontend_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def track(self, params, img, img_id, T_world_cam, is_poseframe):
        """One frame.  `img`: H x W uint8 (any row stride); returns the emitted features as a dict of arrays
        (vtx n x 2, idepth_mu, idepth_var, slot, status)."""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2 or img.shape != (self.H, self.W) or img.strides[1] != 1 or img.strides[0] < self.W:
            raise ValueError("img must be H x W uint8 with unit pixel stride")
        T = _pose(T_world_cam)
        n = C.c_int32()
        _l.check(self._lib.flame_hip_frontend_track(self._h, C.byref(params), C.c_void_p(img.ctypes.data), int(img.strides[0]),
                                                    int(img_id), _ptr(T), int(bool(is_poseframe)), C.byref(n)),
                 "flame_hip_frontend_track")
        return self.features(n.value)

    def set_camera(self, raw_width=None, raw_height=None, D=(0, 0, 0, 0, 0), format=_l.PIX_GRAY8, resize_factor=1):
        """Sets the camera of the ingest stage (raw size, pixel format, integer resize factor, D = k1 k2 p1 p2 k3; the
        handle's K is the K of the output image).  `set_camera(None)`: back to rectified input."""
        if raw_width is None:
            _l.check(self._lib.flame_hip_frontend_set_camera(self._h, None), "flame_hip_frontend_set_camera")
            self._cam = None
            return
        cam = Camera(int(raw_width), int(raw_height), int(format), int(resize_factor), (C.c_float * 5)(*[float(d) for d in D]))
        _l.check(self._lib.flame_hip_frontend_set_camera(self._h, C.byref(cam)), "flame_hip_frontend_set_camera")
        self._cam = cam

    def set_gates(self, letterbox=False, min_height=None, max_height=None, up=(0, -1, 0)):
        """The gates of the frames to come: `letterbox` keeps features in the middle third of the rows; a `min_height` and / or
        `max_height` holds back every tracked feature whose world point lies outside that band along `up` (not normalised;
        (0, -1, 0) for a right-down-forward world).  `set_gates()`: none."""
        height = min_height is not None or max_height is not None
        if not letterbox and not height:
            _l.check(self._lib.flame_hip_frontend_set_gates(self._h, None), "flame_hip_frontend_set_gates")
            return
        big = float(np.finfo(np.float32).max)
        g = Gates(int(bool(letterbox)), int(height), -big if min_height is None else float(min_height),
                  big if max_height is None else float(max_height), (C.c_float * 3)(*[float(a) for a in up]))
        _l.check(self._lib.flame_hip_frontend_set_gates(self._h, C.byref(g)), "flame_hip_frontend_set_gates")

    def set_cost(self, zero_mean=True):
        """The matching cost of the frames to come: COST_ZSSD (zero-mean: bit-invariant to a grey offset between the pose frame
        and the current image -- auto-exposure cameras; wants win_size >= 7 on smooth imagery) or, `zero_mean=False`, COST_SSD
        (the default).  May change between any two frames."""
        _l.check(self._lib.flame_hip_frontend_set_cost(self._h, COST_ZSSD if zero_mean else COST_SSD), "flame_hip_frontend_set_cost")

    def set_gain_invariant(self, on=True):
        """The gain-invariant matching cost for the frames to come: the residual of the reference window after the best fit
        ref ~ g cur + b -- bit-invariant to a power-of-two gain and any offset on the frames tracked against a pose frame that clip
        nowhere; an exposure step (a gain) is what it is for.  While on it overrides `set_cost`; `on=False` returns to that
        choice.  May change between any two frames."""
        _l.check(self._lib.flame_hip_frontend_set_gain_invariant(self._h, 1 if on else 0), "flame_hip_frontend_set_gain_invariant")

    def set_warp(self, on=True):
        """The warped matching window for the frames to come: the current image is sampled where the reference window's pixels land
        under the pose change (an affine map per feature and frame, taken at the prior) -- for cameras that roll or change their
        distance against the pose frame.  A feature whose map is out of range (a stretch above 4, an area scale below 1/16,
        mirrored) is refused: OUTSIDE, counted in info key "warp_refused".  Under a pure sideways translation it changes no bit.
        May change between any two frames."""
        _l.check(self._lib.flame_hip_frontend_set_warp(self._h, 1 if on else 0), "flame_hip_frontend_set_warp")

    def set_carry(self, on=True):
        """The hand-over for the pose frames to come: when a pose frame takes a ring slot that is in use, the features of the pose
        frame it evicts are tracked against the new image once more instead of dying; those the frame emits (status OK or
        NO_PARALLAX, winner of their cell) at a pixel where a detection could sit are re-anchored in the new pose frame at that
        pixel, with the emitted inverse depth and variance as their prior; the others die behind the frame.  For cameras that
        hover.  Info keys "carried", "carry_lost" (of the last frame).  May change between any two frames."""
        _l.check(self._lib.flame_hip_frontend_set_carry(self._h, 1 if on else 0), "flame_hip_frontend_set_carry")

    def set_ref_grad(self, min_grad):
        """The reference-patch gradient gate of the frames to come: a feature whose reference window has a root-mean-square grey
        gradient below `min_grad` ALONG its epipolar line (an edge parallel to the line: the aperture problem) is not searched and
        gets status REF_GRAD, a failure like AMBIGUOUS.  0 (the default) switches it off.  May change between any two frames."""
        _l.check(self._lib.flame_hip_frontend_set_ref_grad(self._h, float(min_grad)), "flame_hip_frontend_set_ref_grad")

    def _raw(self, raw):
        cam = getattr(self, "_cam", None)
        raw = np.asarray(raw)
        if cam is None:  # (the library refuses the call with STATE before it reads the image)
            return np.ascontiguousarray(raw, np.uint8)
        ch = PIX_CHANNELS[cam.format]
        shape = (cam.raw_height, cam.raw_width) + ((ch,) if ch > 1 else ())
        if raw.dtype != np.uint8 or raw.shape != shape or raw.strides[1] != ch or (ch > 1 and raw.strides[2] != 1) or \
                raw.strides[0] < cam.raw_width * ch:
            raise ValueError("raw must be raw_height x raw_width%s uint8 with packed pixels" % (" x %d" % ch if ch > 1 else ""))
        return raw

    def track_raw(self, params, raw, img_id, T_world_cam, is_poseframe):
        """`track` with the ingest stage in front: `raw` is the image as the camera delivers it (any row stride)."""
        raw = self._raw(raw)
        T = _pose(T_world_cam)
        n = C.c_int32()
        _l.check(self._lib.flame_hip_frontend_track_raw(self._h, C.byref(params), C.c_void_p(raw.ctypes.data), int(raw.strides[0]),
                                                        int(img_id), _ptr(T), int(bool(is_poseframe)), C.byref(n)),
                 "flame_hip_frontend_track_raw")
        return self.features(n.value)

    def rectify(self, raw):
        """The ingest stage alone: the H x W rectified grey image of `raw`; feature state and ring stay untouched."""
        raw = self._raw(raw)
        out = np.zeros((self.H, self.W), np.uint8)
        _l.check(self._lib.flame_hip_frontend_rectify(self._h, C.c_void_p(raw.ctypes.data), int(raw.strides[0]), _ptr(out), self.W),
                 "flame_hip_frontend_rectify")
        return out

    def image(self):
        """The image the last track / track_raw call tracked (after the ingest stage)."""
        out = np.zeros((self.H, self.W), np.uint8)
        _l.check(self._lib.flame_hip_frontend_image(self._h, _ptr(out), self.W), "flame_hip_frontend_image")
        return out

    def debug_image(self, kind, pitch=None, out=None):
        """The Detections / Matches debug image (IMG_*) of the last tracked frame, rendered on the GPU: (H, W, 3) uint8, BGR.
        `pitch`: bytes between rows (>= 3 W); `out`: a flat uint8 buffer of H x pitch bytes to draw into (the result is a view of
        it; the bytes between the rows are left alone)."""
        pitch = 3 * self.W if pitch is None else int(pitch)
        if out is None:
            out = np.zeros(self.H * max(pitch, 0), np.uint8)
        if out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous or out.size < self.H * pitch:
            raise ValueError("out must be a flat uint8 buffer of H x pitch bytes")
        _l.check(self._lib.flame_hip_frontend_debug_image(self._h, int(kind), _ptr(out), pitch), "flame_hip_frontend_debug_image")
        return np.lib.stride_tricks.as_strided(out, (self.H, self.W, 3), (pitch, 3, 1))

    def searches(self):
        """The search every slot ran in the last frame (debug hook): seg (F, 4) = {x0, y0, ex, ey}, steps (F,) = S, 0 = none."""
        F = self.max_features
        s = dict(seg=np.zeros((F, 4), np.float32), steps=np.zeros(F, np.int32))
        _l.check(self._lib.flame_hip_frontend_searches(self._h, _ptr(s["seg"]), _ptr(s["steps"])), "flame_hip_frontend_searches")
        return s

    def features(self, n=None):
        n = self.info("emitted") if n is None else n
        out = dict(vtx=np.zeros((n, 2), np.float32), idepth_mu=np.zeros(n, np.float32), idepth_var=np.zeros(n, np.float32),
                   slot=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
        _l.check(self._lib.flame_hip_frontend_features(self._h, n, _ptr(out["vtx"]), _ptr(out["idepth_mu"]), _ptr(out["idepth_var"]),
                                                       _ptr(out["slot"]), _ptr(out["status"])), "flame_hip_frontend_features")
        return out

    def set_poses(self, ids, poses):
        ids = np.ascontiguousarray(ids, np.uint32)
        T = np.ascontiguousarray(np.concatenate([_pose(p) for p in poses]) if len(ids) else np.zeros(0))
        _l.check(self._lib.flame_hip_frontend_set_poses(self._h, len(ids), _ptr(ids), _ptr(T)), "flame_hip_frontend_set_poses")

    def prune(self, keep_ids):
        ids = np.ascontiguousarray(keep_ids, np.uint32)
        _l.check(self._lib.flame_hip_frontend_prune(self._h, len(ids), _ptr(ids)), "flame_hip_frontend_prune")

    def info(self, key):
        v = C.c_int64()
        _l.check(self._lib.flame_hip_frontend_info(self._h, key.encode(), C.byref(v)), "flame_hip_frontend_info(%s)" % key)
        return v.value

    def state(self):
        """Every slot's state (debug hook): dict of max_features-long arrays."""
        F = self.max_features
        s = dict(alive=np.zeros(F, np.uint8), u=np.zeros(F, np.int32), v=np.zeros(F, np.int32), pf=np.zeros(F, np.int32),
                 mu=np.zeros(F, np.float32), var=np.zeros(F, np.float32), drop=np.zeros(F, np.int32),
                 status=np.zeros(F, np.int32), kstar=np.zeros(F, np.int32))
        _l.check(self._lib.flame_hip_frontend_state(self._h, *[_ptr(s[k]) for k in ("alive", "u", "v", "pf", "mu", "var", "drop",
                                                                                    "status", "kstar")]), "flame_hip_frontend_state")
        return s
