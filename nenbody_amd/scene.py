"""Host-side mirror of the reference's update interface for the n-body path, over the C ABI.

The reference keeps the simulation state in ``main()`` (``positions``, ``velocities``, ``old_positions``,
``old_velocities``, ``instance_data``: src/main.rs:738-750) and advances it with the free function
``update_instance_nbody`` (src/main.rs:404-441), called once per redraw (call-site shape: src/main.rs:925-931).
Its ``src/scene.rs`` is empty (src/scene.rs:1); :class:`Scene` is the type that module was evidently meant
to hold, and :func:`update_instance_nbody` keeps the reference's own five-argument signature.

Everything here is plumbing (numpy arrays in, ctypes calls, numpy arrays out).  The arithmetic runs in
libnenbody_hip.so on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from ._lib import NB_MODE_FAST, NB_MODE_STRICT, NbBoidsParams, NbError, NbParams, check  # noqa: F401  (re-exported)

__all__ = ["Scene", "update_instance_nbody", "update_instance_boids", "update_release", "init_state", "eye_constant", "eye_sample_offsets", "frame_constant", "frame_sample_offsets", "srgb_decode", "srgb_encode",
           "NB_MODE_STRICT",
           "NB_MODE_FAST", "NbParams", "NbBoidsParams", "NbError"]


def _as_f32(a, shape_tail, name):
    arr = np.ascontiguousarray(a, dtype=np.float32)
    if arr.ndim != len(shape_tail) + 1 or tuple(arr.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name} must have shape (n, {', '.join(map(str, shape_tail))}), got {arr.shape}")
    return arr


def camera_constant(vertical_fov_deg: float, aspect_ratio: float, near: float = 1.0, far: float = 10000.0) -> np.ndarray:
    """The constant of a camera array, OPENGL_TO_WGPU_MATRIX * cgmath::perspective(...) (src/gfx.rs:12-17, 365, 367), as the
    (4, 4) array ``Scene.cameras`` takes ([k] = column k).  The reference's CameraArray::new derives the vertical field of view
    as horizontal_fov / aspect_ratio (src/gfx.rs:381) and build_camera passes near = 1, far = 10000."""
    cp = np.zeros((4, 4), np.float32)
    check(_lib.load().nb_camera_constant(vertical_fov_deg, aspect_ratio, near, far, cp.ctypes.data))
    return cp


def eye_constant(width: int = 1024, horizontal_fov_deg: float = 90.0) -> np.ndarray:
    """The constant of the reference's eye cameras for rows of ``width`` pixels, as it forms it: CameraArray::new takes the
    horizontal field of view and an extent of width x 1 (src/main.rs:693-697) and passes perspective() the angle DIVIDED by the
    aspect ratio (src/gfx.rs:379-383), so a row spans 2 atan(width tan(fov / (2 width))) -- 76.3 degrees at 90 and 1024, not 90."""
    w = np.float32(width)
    return camera_constant(float(np.float32(horizontal_fov_deg) / w), float(w / np.float32(1.0)), 1.0, 10000.0)


def frame_constant(extent=(1920, 1080), horizontal_fov_deg: float = 90.0) -> np.ndarray:
    """The constant of the reference's scene camera for a target of ``extent`` = (width, height) pixels, as it forms it
    (src/main.rs:753-762): the aspect ratio a = (float)width / (float)height, and perspective() given the angle DIVIDED by it
    (src/gfx.rs:379-383; kept, as for the eyes): camera_constant(fov / a, a, 1, 10000)."""
    a = np.float32(extent[0]) / np.float32(extent[1])
    return camera_constant(float(np.float32(horizontal_fov_deg) / a), float(a), 1.0, 10000.0)


def eye_sample_offsets() -> np.ndarray:
    """Where the eight samples of a column lie, as fractions of the column (nb_eyes_sample_offsets): sample k of column c is at
    c + o[k], o = (9, 7, 13, 5, 3, 1, 11, 15) / 16, the x coordinates of Vulkan's standard 8-sample pattern."""
    out = np.empty(_lib.NB_EYES_SAMPLES, np.float32)
    check(_lib.load().nb_eyes_sample_offsets(out.ctypes.data))
    return out


def frame_sample_offsets() -> np.ndarray:
    """Where the eight samples of a pixel lie, as fractions of the pixel (nb_frame_sample_offsets): sample k of pixel (c, r) is at
    (c + o[0, k], r + o[1, k]), o[0] = :func:`eye_sample_offsets`, o[1] = (5, 11, 9, 3, 13, 7, 15, 1) / 16 -- Vulkan's standard
    8-sample pattern.  Returns (2, 8)."""
    out = np.empty((2, _lib.NB_EYES_SAMPLES), np.float32)
    check(_lib.load().nb_frame_sample_offsets(out.ctypes.data))
    return out


def srgb_decode(srgb8) -> np.ndarray:
    """8-bit sRGB values as the linear binary32 a Rgba8UnormSrgb texture hands the shader: the library's table
    D[b] = binary32(decode(b / 255)) (nb_srgb_decode_table).  Same shape as ``srgb8`` (uint8)."""
    table = np.empty(256, np.float32)
    check(_lib.load().nb_srgb_decode_table(table.ctypes.data))
    return table[np.asarray(srgb8, np.uint8)]


def srgb_encode(linear) -> np.ndarray:
    """Linear values as the bytes an sRGB target stores (nb_srgb_encode): the exact nearest byte, table-driven; a NaN gives 0.
    Same shape as ``linear``, uint8."""
    lin = np.ascontiguousarray(linear, np.float32)
    out = np.empty(lin.shape, np.uint8)
    check(_lib.load().nb_srgb_encode(lin.ctypes.data, lin.size, out.ctypes.data))
    return out


def init_state(n: int, seed: int = 1234):
    """Seeded stand-in for the reference's unseeded initial state (src/main.rs:736-747).

    Returns (positions, velocities), float32 arrays of shape (n, 3): velocities (U[0,0.1), U[0,0.1), 0)
    drawn first for every body, then positions (U[-100,100), U[-100,100), 0) -- the reference's
    distributions and draw order.
    """
    pos = np.empty((n, 3), np.float32)
    vel = np.empty((n, 3), np.float32)
    check(_lib.load().nb_init_state(seed, n, pos.ctypes.data, vel.ctypes.data))
    return pos, vel


# the arrays an eye-row entry fills (Scene._eye_rows): (dtype, shape behind (count, width)), None for one word an eye
_PER_EYE, _U32, _F32, _RGBA = (np.uint32, None), (np.uint32, ()), (np.float32, ()), (np.float32, (4,))


class Scene:
    """Device-resident n-body state with the update of src/main.rs:404-441 as :meth:`step`.

    Host mirrors (``positions``, ``velocities``, ``instances``) are refreshed by :meth:`step`, so the
    consumers at src/main.rs:932-945 (instance upload, cameras) would read them unchanged;
    :meth:`step_n` keeps everything on the device and is the benchmark path.
    """

    def __init__(self, positions, velocities, params: Optional[NbParams] = None):
        lib = _lib.load()
        pos = _as_f32(positions, (3,), "positions")
        vel = _as_f32(velocities, (3,), "velocities")
        if len(pos) != len(vel):
            raise ValueError("positions and velocities must have the same length")
        if len(pos) == 0:
            raise ValueError("a Scene needs at least one body")
        self.n = len(pos)
        self.params = params if params is not None else _lib.default_params()
        self._lib = lib
        self._ctx = ctypes.c_void_p()
        check(lib.nb_create(self.n, 1, ctypes.byref(self.params), ctypes.byref(self._ctx)))
        self._positions = pos.copy()
        self._velocities = vel.copy()
        self._instances = np.zeros((self.n, 4, 4), np.float32)
        try:
            check(lib.nb_upload(self._ctx, self._positions.ctypes.data, self._velocities.ctypes.data), self._ctx)
        except Exception:
            self.close()
            raise

    # -- constructors mirroring the Rust shim ---------------------------------------
    @classmethod
    def new(cls, n: int, params: Optional[NbParams] = None, seed: int = 1234) -> "Scene":
        pos, vel = init_state(n, seed)
        return cls(pos, vel, params)

    @classmethod
    def from_state(cls, positions, velocities, params: Optional[NbParams] = None) -> "Scene":
        return cls(positions, velocities, params)

    # -- stepping ---------------------------------------------------------------------------------------
    def step(self) -> None:
        """One update_instance_nbody, then refresh the host mirrors (positions, velocities, instances)."""
        check(self._lib.nb_step(self._ctx, 1), self._ctx)
        self._refresh(True)

    def step_n(self, k: int) -> None:
        """k updates, device-resident and asynchronous; host mirrors are NOT refreshed (see :meth:`sync`)."""
        check(self._lib.nb_step(self._ctx, int(k)), self._ctx)

    def step_boids(self, params: Optional[NbBoidsParams] = None) -> None:
        """One update_instance_boids (src/main.rs:443-526), then refresh the host mirrors."""
        check(self._lib.nb_step_boids(self._ctx, 1, ctypes.byref(params) if params is not None else None), self._ctx)
        self._refresh(True)

    def step_boids_n(self, k: int, params: Optional[NbBoidsParams] = None) -> None:
        """k boids updates, device-resident and asynchronous; host mirrors are NOT refreshed."""
        check(self._lib.nb_step_boids(self._ctx, int(k), ctypes.byref(params) if params is not None else None), self._ctx)

    def step_random(self, seed: int = 0, k: int = 1) -> None:
        """k random-walk updates (update_instance_random, src/main.rs:381-402), then refresh the host mirrors."""
        check(self._lib.nb_step_random(self._ctx, int(k), int(seed)), self._ctx)
        self._refresh(True)

    def cameras(self, up, cp) -> np.ndarray:
        """CameraArray::update (src/gfx.rs:397-408) for the current state: per body cp * look_at_dir(position, velocity,
        up).  ``cp`` is the array's constant correction*proj as a (4, 4) array whose [k] is column k.  Returns (n, 4, 4)."""
        upv = np.ascontiguousarray(up, np.float32).reshape(3)
        cpm = np.ascontiguousarray(cp, np.float32).reshape(16)
        out = np.zeros((self.n, 4, 4), np.float32)
        check(self._lib.nb_cameras(self._ctx, upv.ctypes.data, cpm.ctypes.data, out.ctypes.data), self._ctx)
        return out

    def eyes(self, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None, first: int = 0, count: Optional[int] = None,
             see_self: bool = False):
        """Every entity's eye view (nb_eyes) for bodies [first, first + count) of the current state: what the
        reference's depth attachment holds after its eye pass, one row of ``width`` pixels per entity, and which entity wrote each
        pixel.  ``cp`` is the eyes' camera constant, (4, 4) with [k] = column k; None: the reference's, :func:`eye_constant`.
        Returns (ids uint32 (count, width) -- NB_EYES_NONE where nothing covers the column --, depth float32 (count, width))."""
        return self._eye_rows(self._lib.nb_eyes, (_U32, _F32), width, up, cp, first, count, see_self)

    def _eye_setup(self, width, up, cp, max_width=_lib.NB_EYES_MAX_WIDTH):
        if cp is None:   # (an invalid width is the library's to refuse)
            cp = eye_constant(width) if 0 < width <= max_width else np.zeros((4, 4), np.float32)
        return np.ascontiguousarray(up, np.float32).reshape(3), np.ascontiguousarray(cp, np.float32).reshape(16)

    def _eye_rows(self, entry, outputs, width, up, cp, first, count, see_self, max_width=_lib.NB_EYES_MAX_WIDTH):
        """What the eye-row methods share: the defaults of ``count`` and ``cp``, the arrays ``entry`` fills -- one per (dtype, tail)
        of ``outputs``, shaped (count, width) + tail, or (count,) where tail is None -- and the call.  Returns those arrays."""
        if count is None:
            count = self.n - first
        if first < 0 or count < 0:
            raise ValueError("first and count must be >= 0")
        upv, cpm = self._eye_setup(width, up, cp, max_width)
        w = max(int(width), 0)
        out = tuple(np.empty((count,) if tail is None else (count, w) + tail, dtype) for dtype, tail in outputs)
        flags = _lib.NB_EYES_SEE_SELF if see_self else 0
        check(entry(self._ctx, first, count, upv.ctypes.data, cpm.ctypes.data, width, flags, *(a.ctypes.data for a in out)), self._ctx)
        return out

    def seen(self, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None, first: int = 0, count: Optional[int] = None,
             see_self: bool = False):
        """The seen set of every eye (nb_eyes_seen) for bodies [first, first + count) of the current state: which
        entities occur in the eye's row of :meth:`eyes` (same arguments), in ascending order, with the nearest depth and the number of
        columns of each.  Returns (count uint32 (count,), ids uint32 (count, width) -- NB_EYES_NONE behind the first count[e] slots --,
        depth float32 (count, width) -- 1.0 there --, cols uint32 (count, width) -- 0 there)."""
        return self._eye_rows(self._lib.nb_eyes_seen, (_PER_EYE, _U32, _F32, _U32), width, up, cp, first, count, see_self)

    def step_boids_seen(self, params: Optional[NbBoidsParams] = None, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None,
                        batch: int = 0) -> None:
        """One update_instance_boids restricted to what each entity sees (nb_step_boids_seen): body n folds
        over the entities of its own eye row of :meth:`eyes` instead of over every entity; one that sees nobody stops.  Then refresh
        the host mirrors.  ``batch``: eyes processed at a time (0: the library's choice); every value gives the same bits."""
        self.step_boids_seen_n(1, params, width, up, cp, batch)
        self._refresh(True)

    def step_boids_seen_n(self, k: int, params: Optional[NbBoidsParams] = None, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None,
                          batch: int = 0) -> None:
        """k such updates, device-resident and asynchronous; host mirrors are NOT refreshed."""
        upv, cpm = self._eye_setup(width, up, cp)
        check(self._lib.nb_step_boids_seen(self._ctx, int(k), ctypes.byref(params) if params is not None else None, upv.ctypes.data,
                                           cpm.ctypes.data, width, int(batch)), self._ctx)

    def located(self, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None, first: int = 0, count: Optional[int] = None,
                see_self: bool = False):
        """Where every eye sees the members of its seen set (nb_eyes_located) for bodies [first, first + count)
        of the current state: per member of :meth:`seen` (same arguments) the column at which it is nearest and the seen point relative
        to the eye in world axes, formed from the eye's row, its heading, ``up`` and ``cp`` alone.  ``cp`` must be a perspective
        constant as :func:`camera_constant` forms it.  Returns (count, ids, depth, cols as :meth:`seen`, col uint32 (count, width) --
        NB_EYES_NONE behind the first count[e] slots --, rel float32 (count, width, 4) -- (x, y, z, range), +0 there)."""
        return self._eye_rows(self._lib.nb_eyes_located, (_PER_EYE, _U32, _F32, _U32, _U32, _RGBA), width, up, cp, first, count, see_self)

    def step_nbody_located(self, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None, batch: int = 0) -> None:
        """One update_instance_nbody from vision alone (nb_step_nbody_located): body n folds the reference's
        law over the relative positions of :meth:`located` instead of over p_i - p_n; one that sees nobody coasts.  Then refresh the
        host mirrors.  ``batch``: eyes processed at a time (0: the library's choice); every value gives the same bits."""
        self.step_nbody_located_n(1, width, up, cp, batch)
        self._refresh(True)

    def step_nbody_located_n(self, k: int, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None, batch: int = 0) -> None:
        """k such updates, device-resident and asynchronous; host mirrors are NOT refreshed."""
        upv, cpm = self._eye_setup(width, up, cp)
        check(self._lib.nb_step_nbody_located(self._ctx, int(k), upv.ctypes.data, cpm.ctypes.data, width, int(batch)), self._ctx)

    def set_skin(self, rgba=None) -> None:
        """The skin the colour rows sample (nb_eyes_skin): an array (th, tw, 4), row 0 first as the image file stores it -- floats
        are linear RGBA, uint8 is an sRGB image (Rgba8UnormSrgb: colour through :func:`srgb_decode`, alpha / 255).  None: the 1 x 1
        white skin, which gives the pure vignette."""
        if rgba is None:
            check(self._lib.nb_eyes_skin(self._ctx, None, 0, 0), self._ctx)
            return
        a = np.asarray(rgba)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError(f"a skin must have shape (th, tw, 4), got {a.shape}")
        if a.dtype == np.uint8:
            lin = np.empty(a.shape, np.float32)
            lin[..., :3] = srgb_decode(a[..., :3])
            lin[..., 3] = a[..., 3].astype(np.float32) / np.float32(255)
        else:
            lin = np.ascontiguousarray(a, np.float32)
        check(self._lib.nb_eyes_skin(self._ctx, lin.ctypes.data, a.shape[1], a.shape[0]), self._ctx)

    def eyes_colour(self, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None, first: int = 0, count: Optional[int] = None,
                    see_self: bool = False):
        """:meth:`eyes` with the colour row of the same pass (nb_eyes_colour): per column the
        winning fragment's texel of the skin (:meth:`set_skin`) under the vignette, or the clear colour.
        Returns (ids, depth, rgba float32 (count, width, 4) linear, bgra8 uint32 (count, width) whose bytes are B, G, R, A: the
        texel of the reference's Bgra8UnormSrgb target)."""
        return self._eye_rows(self._lib.nb_eyes_colour, (_U32, _F32, _RGBA, _U32), width, up, cp, first, count, see_self)

    def eyes_msaa(self, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None, first: int = 0, count: Optional[int] = None,
                  see_self: bool = False):
        """The eye rows through 8 samples per column, resolved as the reference's targets are (nb_eyes_msaa, DESIGN.md section 10
        steps M1-M5): sample k of column c lies at c + :func:`eye_sample_offsets` [k]; a column's colour is the mean of its samples'
        fragments (one fragment per column, body and edge, shaded at the column centre) and of the clear colour where a sample is
        empty.  ``width`` is at most NB_EYES_MSAA_MAX_WIDTH.
        Returns (ids8 uint32 (count, width, 8), depth8 float32 (count, width, 8), rgba float32 (count, width, 4) linear, bgra8
        uint32 (count, width) whose bytes are B, G, R, A)."""
        samples = (_lib.NB_EYES_SAMPLES,)
        return self._eye_rows(self._lib.nb_eyes_msaa, ((np.uint32, samples), (np.float32, samples), _RGBA, _U32), width, up, cp, first,
                              count, see_self, _lib.NB_EYES_MSAA_MAX_WIDTH)

    def viewport(self, camera: int, scale: float = 0.1, extent=(1024, 768), width: int = 1024, up=(0.0, 0.0, 1.0), cp=None,
                 see_self: bool = False, msaa: bool = False) -> np.ndarray:
        """The image the reference's UI shows (src/main.rs:86-96, 981-998): entity ``camera``'s row, a 1-D line of pixels scaled
        to extent * scale.  Returns uint32 (max(1, int(extent[1] * scale)), max(1, int(extent[0] * scale))), bytes B, G, R, A:
        every line is the eye's bgra8 row, image column x showing row column floor((x + 0.5) * width / columns).  ``msaa``: the
        row resolved from 8 samples per column (:meth:`eyes_msaa`), as the reference's is, not the one-sample row."""
        cols = max(1, int(extent[0] * scale))
        rows = max(1, int(extent[1] * scale))
        row = (self.eyes_msaa if msaa else self.eyes_colour)(width, up, cp, camera, 1, see_self)[3][0]
        pick = ((2 * np.arange(cols, dtype=np.int64) + 1) * width) // (2 * cols)
        return np.repeat(row[pick][None, :], rows, 0)

    def camera_at(self, eye, direction, up, cp) -> np.ndarray:
        """One camera from an eye and a direction given by the host (nb_camera_at): cp * look_at_dir(eye, direction, up), formed by
        the kernel behind :meth:`cameras`.  Returns (4, 4), [k] = column k."""
        ev = np.ascontiguousarray(eye, np.float32).reshape(3)
        dv = np.ascontiguousarray(direction, np.float32).reshape(3)
        upv = np.ascontiguousarray(up, np.float32).reshape(3)
        cpm = np.ascontiguousarray(cp, np.float32).reshape(16)
        out = np.zeros((4, 4), np.float32)
        check(self._lib.nb_camera_at(self._ctx, ev.ctypes.data, dv.ctypes.data, upv.ctypes.data, cpm.ctypes.data, out.ctypes.data),
              self._ctx)
        return out

    def scene_camera(self, extent=(1920, 1080), height: float = 990.0, follow: int = 0, cp=None) -> np.ndarray:
        """The reference's scene camera for the current state (src/main.rs:753-762, 940-942): the eye ``height`` above body
        ``follow``, looking down -z with +x up; ``cp`` None: :func:`frame_constant` of ``extent``.  Returns (4, 4)."""
        p = self.positions()[follow]
        if cp is None:
            cp = frame_constant(extent)
        return self.camera_at((p[0], p[1], height), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), cp)

    def frame(self, camera=None, extent=(1920, 1080)):
        """The scene camera's frame (nb_frame): what the reference's display pass leaves in its target of
        ``extent`` = (width, height) pixels, and which entity wrote each pixel.  ``camera``: (4, 4) with [k] = column k; None: the
        reference's, :meth:`scene_camera` of ``extent``.  The skin is :meth:`set_skin`'s.
        Returns (ids uint32 (H, W) -- NB_EYES_NONE where nothing is drawn --, depth float32 (H, W), rgba float32 (H, W, 4) linear,
        bgra8 uint32 (H, W) whose bytes are B, G, R, A); row 0 is the top."""
        w, h = int(extent[0]), int(extent[1])
        if camera is None:   # (an invalid extent is the library's to refuse)
            camera = self.scene_camera((w, h)) if w > 0 and h > 0 else np.zeros((4, 4), np.float32)
        cam = np.ascontiguousarray(camera, np.float32).reshape(16)
        shape = (max(h, 0), max(w, 0))
        ids = np.empty(shape, np.uint32)
        depth = np.empty(shape, np.float32)
        rgba = np.empty(shape + (4,), np.float32)
        bgra8 = np.empty(shape, np.uint32)
        check(self._lib.nb_frame(self._ctx, cam.ctypes.data, max(w, 0), max(h, 0), 0, ids.ctypes.data, depth.ctypes.data,
                                 rgba.ctypes.data, bgra8.ctypes.data), self._ctx)
        return ids, depth, rgba, bgra8

    def frame_msaa(self, camera=None, extent=None):
        """The scene camera's frame through 8 samples per pixel, resolved as the reference's target is (nb_frame_msaa, DESIGN.md
        section 11.1 steps FM1-FM5): sample k of pixel (c, r) lies at (c, r) + :func:`frame_sample_offsets` [:, k]; a pixel's colour
        is the mean of its samples' fragments (one fragment per pixel, body and edge, shaded at the pixel centre) and of the clear
        colour where a sample is empty.  ``camera`` and ``extent`` as :meth:`frame`'s (None: the reference's camera, 1920 x 1080);
        each side of ``extent`` is at most NB_FRAME_MSAA_MAX_DIM.
        Returns (ids8 uint32 (H, W, 8), depth8 float32 (H, W, 8), rgba float32 (H, W, 4) linear, bgra8 uint32 (H, W) whose bytes
        are B, G, R, A); row 0 is the top."""
        if extent is None:
            extent = (1920, 1080)
        w, h = int(extent[0]), int(extent[1])
        if camera is None:   # (an invalid extent is the library's to refuse)
            camera = self.scene_camera((w, h)) if w > 0 and h > 0 else np.zeros((4, 4), np.float32)
        cam = np.ascontiguousarray(camera, np.float32).reshape(16)
        ok = 0 < w <= _lib.NB_FRAME_MSAA_MAX_DIM and 0 < h <= _lib.NB_FRAME_MSAA_MAX_DIM
        shape = (h, w) if ok else (0, 0)   # (nothing is allocated for an extent the library refuses)
        ids8 = np.empty(shape + (_lib.NB_EYES_SAMPLES,), np.uint32)
        depth8 = np.empty(shape + (_lib.NB_EYES_SAMPLES,), np.float32)
        rgba = np.empty(shape + (4,), np.float32)
        bgra8 = np.empty(shape, np.uint32)
        check(self._lib.nb_frame_msaa(self._ctx, cam.ctypes.data, max(w, 0), max(h, 0), 0, ids8.ctypes.data, depth8.ctypes.data,
                                      rgba.ctypes.data, bgra8.ctypes.data), self._ctx)
        return ids8, depth8, rgba, bgra8

    def device_state(self, with_instances: bool = True):
        """Device pointers (ints) of the current position records, velocity records and model matrices: the zero-copy
        hand-off.  Valid until the next step / upload / close."""
        p, v, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(self._lib.nb_device_state(self._ctx, ctypes.byref(p), ctypes.byref(v), ctypes.byref(m) if with_instances else None),
              self._ctx)
        return p.value, v.value, (m.value if with_instances else None)

    def sync(self) -> None:
        check(self._lib.nb_sync(self._ctx), self._ctx)

    @property
    def steps_done(self) -> int:
        return int(self._lib.nb_steps_done(self._ctx))

    # -- state access -----------------------------------------------------------------------------------
    def _refresh(self, with_instances: bool) -> None:
        inst = self._instances.ctypes.data if with_instances else None
        check(self._lib.nb_download(self._ctx, self._positions.ctypes.data, self._velocities.ctypes.data, inst), self._ctx)

    def positions(self) -> np.ndarray:
        self._refresh(False)
        return self._positions

    def velocities(self) -> np.ndarray:
        self._refresh(False)
        return self._velocities

    def instances(self) -> np.ndarray:
        """Model matrices of the current state, shape (n, 4, 4); [k] is column k (column-major, main.rs:437-439)."""
        self._refresh(True)
        return self._instances

    def state(self):
        self._refresh(False)
        return self._positions.copy(), self._velocities.copy()

    # -- lifetime ---------------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.nb_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def policy_floats(features: int, hidden: int) -> int:
    """The floats of one policy of shape (features, hidden) (nb_policy_floats): 0 for a shape outside the limits."""
    if features < 0 or hidden < 0 or features > 0xFFFFFFFF or hidden > 0xFFFFFFFF:
        return 0
    return int(_lib.load().nb_policy_floats(int(features), int(hidden)))


def pack_policy(w1, b1, w2, b2) -> np.ndarray:
    """One policy in the layout :meth:`SceneBatch.set_policy` takes: w1 (F, H) feature-major, b1 (H,), w2 (2, H), b2 (2,) ->
    F*H + H + 2*H + 2 float32."""
    w1 = np.ascontiguousarray(w1, np.float32)
    if w1.ndim != 2:
        raise ValueError("w1 must have shape (features, hidden)")
    hidden = w1.shape[1]
    b1, w2, b2 = (np.ascontiguousarray(a, np.float32) for a in (b1, w2, b2))
    if b1.shape != (hidden,) or w2.shape != (2, hidden) or b2.shape != (2,):
        raise ValueError("b1 must have shape (hidden,), w2 (2, hidden) and b2 (2,)")
    return np.concatenate([w1.reshape(-1), b1, w2.reshape(-1), b2])


def policy_recurrent_floats(features: int, hidden: int) -> int:
    """The floats of one recurrent policy of shape (features, hidden) (nb_policy_recurrent_floats): 0 for a shape outside the limits."""
    if features < 0 or hidden < 0 or features > 0xFFFFFFFF or hidden > 0xFFFFFFFF:
        return 0
    return int(_lib.load().nb_policy_recurrent_floats(int(features), int(hidden)))


def pack_policy_recurrent(w1, wr, b1, w2, b2) -> np.ndarray:
    """One recurrent policy in the layout :meth:`SceneBatch.set_policy_recurrent` takes (R1): w1 (F, H) feature-major, wr (H, H)
    with wr[r, j] the weight of memory word r into hidden unit j, b1 (H,), w2 (2, H), b2 (2,) -> F*H + H*H + H + 2*H + 2 float32."""
    w1 = np.ascontiguousarray(w1, np.float32)
    if w1.ndim != 2:
        raise ValueError("w1 must have shape (features, hidden)")
    hidden = w1.shape[1]
    wr, b1, w2, b2 = (np.ascontiguousarray(a, np.float32) for a in (wr, b1, w2, b2))
    if wr.shape != (hidden, hidden) or b1.shape != (hidden,) or w2.shape != (2, hidden) or b2.shape != (2,):
        raise ValueError("wr must have shape (hidden, hidden), b1 (hidden,), w2 (2, hidden) and b2 (2,)")
    return np.concatenate([w1.reshape(-1), wr.reshape(-1), b1, w2.reshape(-1), b2])


# struct nb_scene_score (include/nenbody.h, Q7): what :meth:`SceneBatch.scores` returns, one record a scene
SCORE_DTYPE = np.dtype([("near", np.uint64), ("spread", np.float32), ("speed2", np.float32), ("momentum2", np.float32),
                        ("goal2", np.float32), ("steps", np.uint32), ("nonfinite", np.uint32)])

# struct nb_es_report (include/nenbody.h, section 14.6): what :meth:`SceneBatch.es_result` returns first
ES_REPORT_DTYPE = np.dtype([("best_scene", np.uint32), ("best_fitness", np.float32), ("nan_count", np.uint32), ("generation", np.uint32)])


class SceneBatch:
    """B independent scenes of n <= NB_SCENES_MAX_BODIES bodies, device-resident, stepped k times by ONE launch with one workgroup
    per scene.  Every scene gets the bits a :class:`Scene` of its n bodies gets.  ``positions`` and
    ``velocities`` have shape (B, n, 3); steps are asynchronous on the batch's stream, the accessors wait."""

    def __init__(self, positions, velocities, params: Optional[NbParams] = None):
        lib = _lib.load()
        pos = np.ascontiguousarray(positions, np.float32)
        vel = np.ascontiguousarray(velocities, np.float32)
        if pos.ndim != 3 or pos.shape[2] != 3 or vel.shape != pos.shape:
            raise ValueError("positions and velocities must both have shape (scenes, n, 3)")
        self.scenes, self.n = int(pos.shape[0]), int(pos.shape[1])
        self.params = params if params is not None else _lib.default_params()
        self._lib = lib
        self._ctx = ctypes.c_void_p()
        self._policy_shape, self._es_floats = (0, 0), 0   # what set_policy and es_set leave
        self._check(lib.nb_scenes_create(self.scenes, self.n, ctypes.byref(self.params), ctypes.byref(self._ctx)), created=False)
        try:
            self._check(lib.nb_scenes_upload(self._ctx, pos.ctypes.data, vel.ctypes.data))
        except Exception:
            self.close()
            raise

    @classmethod
    def new(cls, scenes: int, n: int, seed: int = 1234, params: Optional[NbParams] = None) -> "SceneBatch":
        """scene s starts from init_state(n, seed + s)"""
        states = [init_state(n, seed + s) for s in range(scenes)]
        return cls(np.stack([p for p, _ in states]) if states else np.zeros((0, n, 3), np.float32),
                   np.stack([v for _, v in states]) if states else np.zeros((0, n, 3), np.float32), params)

    def _check(self, status: int, created: bool = True) -> None:
        if status != _lib.NB_OK:
            msg = self._lib.nb_scenes_last_error(self._ctx if created else None)
            raise NbError(status, msg.decode("utf-8", "replace") if msg else "")

    @staticmethod
    def _scene_range(batch, first_scene: int, scene_count: Optional[int]) -> int:
        """scene_count, None: every scene of ``batch`` from first_scene on; a negative bound is refused here, in front of anything
        that reads the batch"""
        if scene_count is None:
            scene_count = batch.scenes - first_scene
        if first_scene < 0 or scene_count < 0:
            raise ValueError("first_scene and scene_count must be >= 0")
        return scene_count

    def step(self, k: int = 1) -> None:
        """k update_instance_nbody of every scene (STRICT), one launch"""
        self._check(self._lib.nb_scenes_step(self._ctx, int(k)))

    def step_boids(self, k: int = 1, params: Optional[NbBoidsParams] = None) -> None:
        """k update_instance_boids of every scene, one launch"""
        self._check(self._lib.nb_scenes_step_boids(self._ctx, int(k), ctypes.byref(params) if params is not None else None))

    @staticmethod
    def _eye_setup(width, up, cp):
        if cp is None:   # (an invalid width is the library's to refuse)
            cp = eye_constant(width) if 0 < width <= _lib.NB_EYES_MAX_WIDTH else np.zeros((4, 4), np.float32)
        return np.ascontiguousarray(up, np.float32).reshape(3), np.ascontiguousarray(cp, np.float32).reshape(16)

    def step_boids_seen(self, k: int = 1, params: Optional[NbBoidsParams] = None, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None) -> None:
        """k update_instance_boids of every scene restricted to what each entity sees of its own scene (nb_scenes_step_boids_seen,
        DESIGN.md section 14.1): the bits :meth:`Scene.step_boids_seen_n` gives each scene, one fused launch per step for the whole
        batch.  ``cp``: the eyes' camera constant, None: :func:`eye_constant`."""
        upv, cpm = self._eye_setup(width, up, cp)
        self._check(self._lib.nb_scenes_step_boids_seen(self._ctx, int(k), ctypes.byref(params) if params is not None else None,
                                                        upv.ctypes.data, cpm.ctypes.data, width))

    def seen(self, first_scene: int = 0, scene_count: Optional[int] = None, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None):
        """The seen sets :meth:`step_boids_seen` folds over (nb_scenes_eyes_seen) for scenes [first_scene, first_scene + scene_count)
        of the current state: per eye the scene-local ids in its row, ascending.  Returns (count uint32 (S, n), ids uint32
        (S, n, width) -- NB_EYES_NONE behind the first count slots); the words of :meth:`Scene.seen` per scene.  Depths and column
        counts are not kept by the batch's step and are not offered."""
        scene_count = SceneBatch._scene_range(self, first_scene, scene_count)
        upv, cpm = self._eye_setup(width, up, cp)
        count = np.empty((scene_count, self.n), np.uint32)
        ids = np.empty((scene_count, self.n, max(int(width), 0)), np.uint32)
        self._check(self._lib.nb_scenes_eyes_seen(self._ctx, first_scene, scene_count, upv.ctypes.data, cpm.ctypes.data, width,
                                                  count.ctypes.data, ids.ctypes.data))
        return count, ids

    def step_nbody_located(self, k: int = 1, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None) -> None:
        """k update_instance_nbody of every scene from vision alone (nb_scenes_step_nbody_located): the bits
        :meth:`Scene.step_nbody_located_n` gives each scene, one fused launch per step for the whole batch.  ``cp``: the eyes' camera
        constant, a perspective constant as :func:`camera_constant` forms it; None: :func:`eye_constant`."""
        upv, cpm = self._eye_setup(width, up, cp)
        self._check(self._lib.nb_scenes_step_nbody_located(self._ctx, int(k), upv.ctypes.data, cpm.ctypes.data, width))

    def located(self, first_scene: int = 0, scene_count: Optional[int] = None, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None):
        """The located sets :meth:`step_nbody_located` folds over (nb_scenes_eyes_located) for scenes [first_scene, first_scene +
        scene_count) of the current state.  Returns (count uint32 (S, n), ids uint32 (S, n, width), depth float32 (S, n, width), col
        uint32 (S, n, width), rel float32 (S, n, width, 4)): the words of :meth:`Scene.located` per scene, padding included, without
        its column counts, which the batch's step does not keep."""
        scene_count = SceneBatch._scene_range(self, first_scene, scene_count)
        upv, cpm = self._eye_setup(width, up, cp)
        shape = (scene_count, self.n, max(int(width), 0))
        count = np.empty(shape[:2], np.uint32)
        ids, depth, col = np.empty(shape, np.uint32), np.empty(shape, np.float32), np.empty(shape, np.uint32)
        rel = np.empty(shape + (4,), np.float32)
        self._check(self._lib.nb_scenes_eyes_located(self._ctx, first_scene, scene_count, upv.ctypes.data, cpm.ctypes.data, width,
                                                     count.ctypes.data, ids.ctypes.data, depth.ctypes.data, col.ctypes.data,
                                                     rel.ctypes.data))
        return count, ids, depth, col, rel

    def set_policy(self, weights, features: int, hidden: int, accel_limit: float = float("inf")) -> None:
        """The batch's policies (nb_scenes_set_policy): ``weights`` of shape (P, policy_floats(features,
        hidden)), P = 1 (every scene uses policy 0) or the number of scenes (scene s uses policy s), each row laid out as
        :func:`pack_policy` lays it out.  ``accel_limit`` >= 0 clamps the two outputs; inf: no limit.  May be called again."""
        w = np.ascontiguousarray(weights, np.float32)
        if w.ndim != 2 or w.shape[1] != policy_floats(features, hidden) or w.shape[1] == 0:
            raise ValueError("weights must have shape (policies, policy_floats(features, hidden))")
        self._check(self._lib.nb_scenes_set_policy(self._ctx, int(features), int(hidden), int(w.shape[0]), w.ctypes.data, float(accel_limit)))
        self._policy_shape = (int(features), int(hidden))

    def set_policy_recurrent(self, weights, features: int, hidden: int, accel_limit: float = float("inf"),
                             memory_limit: float = float("inf")) -> None:
        """The batch's policies, recurrent (nb_scenes_set_policy_recurrent): ``weights`` of shape (P,
        policy_recurrent_floats(features, hidden)), P = 1 or the number of scenes, each row laid out as
        :func:`pack_policy_recurrent` lays it out.  Every body gets ``hidden`` words of memory, cleared to +0 here; ``memory_limit``
        >= 0 clamps what a step writes to it; inf: no limit.  :meth:`step_policy`, :meth:`step_policy_scored` and
        :meth:`policy_observe` then run the recurrent kernel, until :meth:`set_policy` returns the batch to a feedforward policy."""
        w = np.ascontiguousarray(weights, np.float32)
        if w.ndim != 2 or w.shape[1] != policy_recurrent_floats(features, hidden) or w.shape[1] == 0:
            raise ValueError("weights must have shape (policies, policy_recurrent_floats(features, hidden))")
        self._check(self._lib.nb_scenes_set_policy_recurrent(self._ctx, int(features), int(hidden), int(w.shape[0]), w.ctypes.data,
                                                             float(accel_limit), float(memory_limit)))
        self._policy_shape = (int(features), int(hidden))

    def memory(self, first_scene: int = 0, scene_count: Optional[int] = None) -> np.ndarray:
        """The memory of scenes [first_scene, first_scene + scene_count) (nb_scenes_memory): float32 (S, n, H).  Waits for the
        stream."""
        scene_count = SceneBatch._scene_range(self, first_scene, scene_count)
        out = np.zeros((scene_count, self.n, self._policy_shape[1]), np.float32)
        buf = out if out.size else np.zeros(1, np.float32)
        self._check(self._lib.nb_scenes_memory(self._ctx, first_scene, scene_count, buf.ctypes.data))
        return out

    def set_memory(self, memory) -> None:
        """The memory of the whole batch from the host (nb_scenes_set_memory): float32 (B, n, H), any bit patterns."""
        m = np.ascontiguousarray(memory, np.float32)
        if m.shape != (self.scenes, self.n, self._policy_shape[1]) or m.size == 0:
            raise ValueError("memory must have shape (scenes, n, hidden)")
        self._check(self._lib.nb_scenes_set_memory(self._ctx, m.ctypes.data))

    def memory_reset(self) -> None:
        """The memory of every body set to +0 (nb_scenes_memory_reset), asynchronous.  An upload, :meth:`keep` and :meth:`rewind` do
        not touch the memory."""
        self._check(self._lib.nb_scenes_memory_reset(self._ctx))

    def policy_observe_memory(self, first_scene: int = 0, scene_count: Optional[int] = None, width: int = 1024, up=(0.0, 0.0, 1.0),
                              cp=None):
        """:meth:`policy_observe` for a recurrent policy with the memory the step would write (nb_scenes_eyes_policy_memory), the
        memory itself left as it is.  Returns (features float32 (S, n, F), outputs float32 (S, n, 2), next memory float32
        (S, n, H))."""
        scene_count = SceneBatch._scene_range(self, first_scene, scene_count)
        upv, cpm = self._eye_setup(width, up, cp)
        feat = np.empty((scene_count, self.n, self._policy_shape[0]), np.float32)
        act = np.empty((scene_count, self.n, 2), np.float32)
        mem = np.empty((scene_count, self.n, self._policy_shape[1]), np.float32)
        self._check(self._lib.nb_scenes_eyes_policy_memory(self._ctx, first_scene, scene_count, upv.ctypes.data, cpm.ctypes.data, width,
                                                           feat.ctypes.data, act.ctypes.data, mem.ctypes.data))
        return feat, act, mem

    def step_policy(self, k: int = 1, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None) -> None:
        """k steps of every scene under its policy (nb_scenes_step_policy): each body pools its eye row into the policy's features,
        runs the two-layer network and is pushed along its eye's forward and side axes by the two outputs; one fused launch per step
        for the whole batch.  ``width`` must be a multiple of the policy's features."""
        upv, cpm = self._eye_setup(width, up, cp)
        self._check(self._lib.nb_scenes_step_policy(self._ctx, int(k), upv.ctypes.data, cpm.ctypes.data, width))

    def policy_observe(self, first_scene: int = 0, scene_count: Optional[int] = None, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None):
        """What :meth:`step_policy` computes in front of the actuation (nb_scenes_eyes_policy) for scenes [first_scene, first_scene +
        scene_count) of the current state, without stepping.  Returns (features float32 (S, n, F), outputs float32 (S, n, 2) behind
        the limit)."""
        scene_count = SceneBatch._scene_range(self, first_scene, scene_count)
        upv, cpm = self._eye_setup(width, up, cp)
        feat = np.empty((scene_count, self.n, self._policy_shape[0]), np.float32)
        act = np.empty((scene_count, self.n, 2), np.float32)
        self._check(self._lib.nb_scenes_eyes_policy(self._ctx, first_scene, scene_count, upv.ctypes.data, cpm.ctypes.data, width,
                                                    feat.ctypes.data, act.ctypes.data))
        return feat, act

    def set_score(self, radius_sq: float, goal=(0.0, 0.0, 0.0)) -> None:
        """The batch's score (nb_scenes_set_score): ``radius_sq`` >= 0 is the squared radius below which a pair
        counts as near (inf: every pair), ``goal`` the point whose squared distance is summed.  Allocates one record a scene on first
        use and clears the records.  May be called again."""
        g = np.ascontiguousarray(goal, np.float32)
        if g.shape != (3,):
            raise ValueError("goal must have three components")
        sp = _lib.NbScoreParams(float(radius_sq), (ctypes.c_float * 3)(*g.tolist()))
        self._check(self._lib.nb_scenes_set_score(self._ctx, ctypes.byref(sp)))

    def score(self) -> None:
        """The current snapshot of every scene added to its record (nb_scenes_score): one kernel, asynchronous; every float by a
        stated binary32 order (Q1-Q7 of include/nenbody.h), the same bits from run to run."""
        self._check(self._lib.nb_scenes_score(self._ctx))

    def score_reset(self) -> None:
        """The records cleared (nb_scenes_score_reset), asynchronous.  An upload does not clear them."""
        self._check(self._lib.nb_scenes_score_reset(self._ctx))

    def scores(self, first_scene: int = 0, scene_count: Optional[int] = None) -> np.ndarray:
        """The records of scenes [first_scene, first_scene + scene_count) (nb_scenes_scores): a structured array of dtype
        :data:`SCORE_DTYPE`, 32 bytes a scene.  Waits for the stream."""
        scene_count = SceneBatch._scene_range(self, first_scene, scene_count)
        out = np.zeros(max(scene_count, 1), SCORE_DTYPE)
        self._check(self._lib.nb_scenes_scores(self._ctx, first_scene, scene_count, out.ctypes.data))
        return out[:scene_count]

    def step_policy_scored(self, k: int = 1, width: int = 1024, up=(0.0, 0.0, 1.0), cp=None) -> None:
        """k times :meth:`step_policy` (1) then :meth:`score` (nb_scenes_step_policy_scored): a rollout scored where it runs; read
        :meth:`scores` when it ends."""
        upv, cpm = self._eye_setup(width, up, cp)
        self._check(self._lib.nb_scenes_step_policy_scored(self._ctx, int(k), upv.ctypes.data, cpm.ctypes.data, width))

    def es_set(self, mean, features: int, hidden: int, sigma: float, step: float, coef, seed: int = 0,
               accel_limit: float = float("inf")) -> None:
        """The batch's search (nb_scenes_es_set): ``mean`` of policy_floats(features, hidden) floats is the
        policy the population of at most 4 096 scenes is drawn around, ``sigma`` >= 0 the scale of the draw, ``step`` the update's step
        (learning rate, 1/(B sigma) and the utilities' scale folded in), ``coef`` the six coefficients of the fitness over (near,
        spread, speed2, momentum2, goal2, nonfinite), larger is better, ``seed`` 64 bits.  The generation starts at 0."""
        m = np.ascontiguousarray(mean, np.float32)
        if m.ndim != 1 or m.shape[0] != policy_floats(features, hidden) or m.shape[0] == 0:
            raise ValueError("mean must have shape (policy_floats(features, hidden),)")
        c = np.ascontiguousarray(coef, np.float32)
        if c.shape != (6,):
            raise ValueError("coef must have six components")
        ep = _lib.NbEsParams(float(sigma), float(step), (ctypes.c_float * 6)(*c.tolist()), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._check(self._lib.nb_scenes_es_set(self._ctx, int(features), int(hidden), m.ctypes.data, float(accel_limit), ctypes.byref(ep)))
        self._es_floats = int(m.shape[0])
        self._policy_shape = (int(features), int(hidden))

    def es_set_recurrent(self, mean, features: int, hidden: int, sigma: float, step: float, coef, seed: int = 0,
                         accel_limit: float = float("inf"), memory_limit: float = float("inf")) -> None:
        """:meth:`es_set` over a recurrent policy (nb_scenes_es_set_recurrent): ``mean`` has policy_recurrent_floats(features, hidden)
        floats.  A generation is :meth:`rewind`, :meth:`memory_reset`, :meth:`score_reset`, :meth:`es_perturb`,
        :meth:`step_policy_scored`, :meth:`es_update`: :meth:`rewind` does not touch the memory."""
        m = np.ascontiguousarray(mean, np.float32)
        if m.ndim != 1 or m.shape[0] != policy_recurrent_floats(features, hidden) or m.shape[0] == 0:
            raise ValueError("mean must have shape (policy_recurrent_floats(features, hidden),)")
        c = np.ascontiguousarray(coef, np.float32)
        if c.shape != (6,):
            raise ValueError("coef must have six components")
        ep = _lib.NbEsParams(float(sigma), float(step), (ctypes.c_float * 6)(*c.tolist()), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._check(self._lib.nb_scenes_es_set_recurrent(self._ctx, int(features), int(hidden), m.ctypes.data, float(accel_limit),
                                                         float(memory_limit), ctypes.byref(ep)))
        self._es_floats = int(m.shape[0])
        self._policy_shape = (int(features), int(hidden))

    def es_perturb(self) -> None:
        """The batch's policies become the population of the current generation (nb_scenes_es_perturb): scene s gets
        mean + sigma e(seed, generation, s), scenes 2q and 2q + 1 mirrored.  Asynchronous."""
        self._check(self._lib.nb_scenes_es_perturb(self._ctx))

    def es_update(self) -> None:
        """The score records ranked, the mean moved along the rank-weighted sum of the draws and the generation incremented
        (nb_scenes_es_update).  Asynchronous; needs :meth:`set_score`."""
        self._check(self._lib.nb_scenes_es_update(self._ctx))

    def es_mean(self) -> np.ndarray:
        """The mean (nb_scenes_es_mean): policy_floats float32.  Waits for the stream."""
        out = np.zeros(max(self._es_floats, 1), np.float32)
        self._check(self._lib.nb_scenes_es_mean(self._ctx, out.ctypes.data))
        return out[:self._es_floats]

    def es_result(self):
        """What the last :meth:`es_update` left (nb_scenes_es_result): (report, a record of dtype :data:`ES_REPORT_DTYPE`; fitness
        float32 (B,); rank uint32 (B,), 0 the worst).  Waits for the stream."""
        report = np.zeros((), ES_REPORT_DTYPE)
        fitness, rank = np.zeros(self.scenes, np.float32), np.zeros(self.scenes, np.uint32)
        self._check(self._lib.nb_scenes_es_result(self._ctx, report.ctypes.data, fitness.ctypes.data, rank.ctypes.data))
        return report, fitness, rank

    @property
    def es_generation(self) -> int:
        return int(self._lib.nb_scenes_es_generation(self._ctx))

    def keep(self) -> None:
        """The current positions, velocities and step counter copied to buffers the batch keeps (nb_scenes_keep), on the device."""
        self._check(self._lib.nb_scenes_keep(self._ctx))

    def rewind(self) -> None:
        """The kept state copied back (nb_scenes_rewind).  Asynchronous."""
        self._check(self._lib.nb_scenes_rewind(self._ctx))

    def _download(self, what: int) -> np.ndarray:
        out = np.empty((self.scenes, self.n, 4, 4) if what == 2 else (self.scenes, self.n, 3), np.float32)
        args = [None, None, None]
        args[what] = out.ctypes.data
        self._check(self._lib.nb_scenes_download(self._ctx, *args))
        return out

    def positions(self) -> np.ndarray:
        return self._download(0)

    def velocities(self) -> np.ndarray:
        return self._download(1)

    def instances(self) -> np.ndarray:
        """model matrices of the current state, shape (B, n, 4, 4); [k] is column k"""
        return self._download(2)

    def device_state(self, with_instances: bool = True):
        """Device pointers (ints) of the batch's position records, velocity records and model matrices; scene s starts s * n
        records (matrices) behind each.  Valid until the next step / upload / close."""
        p, v, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.nb_scenes_device_state(self._ctx, ctypes.byref(p), ctypes.byref(v), ctypes.byref(m) if with_instances else None))
        return p.value, v.value, (m.value if with_instances else None)

    def sync(self) -> None:
        self._check(self._lib.nb_scenes_sync(self._ctx))

    @property
    def steps_done(self) -> int:
        return int(self._lib.nb_scenes_steps(self._ctx))

    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.nb_scenes_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _check_update_args(instances, positions, old_positions, velocities, old_velocities):
    for name, arr, tail in (("instances", instances, (4, 4)), ("positions", positions, (3,)),
                            ("old_positions", old_positions, (3,)), ("velocities", velocities, (3,)),
                            ("old_velocities", old_velocities, (3,))):
        if not (isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.flags.c_contiguous and arr.flags.writeable):
            raise TypeError(f"{name} must be a writable C-contiguous float32 numpy array")
        if arr.ndim != len(tail) + 1 or tuple(arr.shape[1:]) != tail:
            raise ValueError(f"{name} must have shape (n, {', '.join(map(str, tail))})")


def _update_call(fn, instances, positions, old_positions, velocities, old_velocities, params):
    _check_update_args(instances, positions, old_positions, velocities, old_velocities)
    args = []
    for arr in (instances, positions, old_positions, velocities, old_velocities):
        args += [arr.ctypes.data if len(arr) else None, len(arr)]
    rc = fn(*args, ctypes.byref(params) if params is not None else None)
    if rc == _lib.NB_ERR_INVALID:  # the reference panics here (copy_from_slice, indexing); in Python that is a ValueError
        raise ValueError(_lib.load().nb_last_error(None).decode())
    check(rc)


def update_instance_boids(instances, positions, old_positions, velocities, old_velocities,
                          params: Optional[NbBoidsParams] = None) -> None:
    """The reference's live controller with its own five arguments, updated in place (src/main.rs:443-449).

    Same contract as :func:`update_instance_nbody` (snapshot copies first, main.rs:459-460; `zip` stops at the
    shortest of instances / positions / velocities, main.rs:465-469).  The position folds run over all of
    ``old_positions`` and the velocity fold (main.rs:494-504) over all of ``old_velocities``, each with its own length.
    One call of ``nb_update_instance_boids`` (include/nenbody.h).
    """
    _update_call(_lib.load().nb_update_instance_boids, instances, positions, old_positions, velocities, old_velocities, params)


def update_instance_nbody(instances, positions, old_positions, velocities, old_velocities,
                          params: Optional[NbParams] = None) -> None:
    """The reference's operator, same five arguments, updated in place (src/main.rs:404-410).

    ``instances`` is (n, 4, 4) float32, the others (n, 3) float32 numpy arrays (they must be writable,
    C-contiguous float32: they are the caller's ``Vec``s).  Behaviour kept from the reference:
      * ``old_positions`` / ``old_velocities`` receive copies of the inputs (main.rs:415-416); a length
        mismatch is an error, as ``copy_from_slice`` panics;
      * ``instances.zip(positions).zip(velocities)`` stops at the shortest of the three (main.rs:420-423):
        only that many bodies are updated, while the fold still runs over all of ``old_positions``.
    One call of ``nb_update_instance_nbody`` (include/nenbody.h): one upload, one step, one download; the device context
    is kept inside the library between calls.  A caller that steps repeatedly without reading the state back should
    hold a :class:`Scene` instead.
    """
    _update_call(_lib.load().nb_update_instance_nbody, instances, positions, old_positions, velocities, old_velocities, params)


def _random_args(instances, positions, velocities):
    for name, arr, tail in (("instances", instances, (4, 4)), ("positions", positions, (3,)), ("velocities", velocities, (3,))):
        if not (isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.flags.c_contiguous and arr.flags.writeable):
            raise TypeError(f"{name} must be a writable C-contiguous float32 numpy array")
        if arr.ndim != len(tail) + 1 or tuple(arr.shape[1:]) != tail:
            raise ValueError(f"{name} must have shape (n, {', '.join(map(str, tail))})")
    args = []
    for arr in (instances, positions, velocities):
        args += [arr.ctypes.data if len(arr) else None, len(arr)]
    return args


def update_instance_random(instances, positions, velocities) -> None:
    """The reference's third controller with its own three arguments, updated in place (src/main.rs:381-385): every body's
    velocity takes a small random kick in x and y, the position follows, the matrix is rebuilt; `zip` stops at the shortest of
    the three (main.rs:386-389).  The reference draws from an unseeded ``thread_rng``; here body n at the k-th call draws from
    the counter-based stream (seed, k, n), seed and call counter kept by the library (:func:`update_random_seed` sets the
    seed and restarts the counter), so a run is reproducible.  One call of ``nb_update_instance_random``."""
    check(_lib.load().nb_update_instance_random(*_random_args(instances, positions, velocities)))


def update_instance_random_seeded(instances, positions, velocities, seed: int = 0, step: int = 0) -> None:
    """:func:`update_instance_random` with the stream position given by the caller: body n draws from (seed, step, n).
    One call of ``nb_update_instance_random_seeded``."""
    check(_lib.load().nb_update_instance_random_seeded(*_random_args(instances, positions, velocities), int(seed), int(step)))


def update_random_seed(seed: int) -> None:
    """Seed of :func:`update_instance_random`'s stream; restarts its call counter."""
    _lib.load().nb_update_random_seed(int(seed))


def update_release() -> None:
    """Frees the device contexts the drop-in functions keep between calls."""
    _lib.load().nb_update_release()
