"""The cameras of the view-set tests (include/rtamd.h: rt_views_*), written for soup_a of surface_cases.py: 300 triangles within about
+-3.5, the scene's own camera at (0, 0, 6), so the walkers' node grid spans about +-3.5 in x and y and -3.5 .. 6 in z, and the query
layer's origin bound is about 6.  The same table serves sphere_emissive_env, the environment instance of the kernel.

  own      the scene's camera: what rt_render itself draws
  inside   (1.5, -1, 4), a rotated orthonormal basis, fov_y 0.6: inside grid and bound, the walkers' case
  within   (0.3, 0.2, 0.1), inside the soup, looking along +x
  skew     right scaled by 1.3 and up not orthogonal to forward: the reference uses the vectors as given
  beside   (5.5, 0, 0) looking along -x: inside the origin bound, outside the node grid in x -- every first ray is the exact role's
  far      (0, 0, 40): beyond the origin bound -- likewise

swapped(sd, camera) rebuilds a SceneData with the camera replaced, the way surface_cases._with rebuilds one: the referee of view v is
a scene created from it."""
import numpy as np

import pin_cases

rt = pin_cases.rt

NAMES = ("own", "inside", "within", "skew", "beside", "far")
SIZES = [(8, 8), (40, 24), (43, 21)]   # one sub-tile; 15 whole sub-tiles; 6 x 3 with padded right and bottom borders
SLICE, DEPTH = 4, 4


def camera(position, right, up, forward, fov_y):
    c = rt.rt_camera()
    for field, v in (("position", position), ("right", right), ("up", up), ("forward", forward)):
        for k in range(3):
            getattr(c, field)[k] = float(np.float32(v[k]))
    c.fov_y = float(np.float32(fov_y))
    return c


def _rotated():
    """An orthonormal basis turned 0.35 about y, then -0.25 about x: it looks from (1.5, -1, 4) towards the soup."""
    a, b = 0.35, -0.25
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = ry @ rx
    return m @ np.array([1.0, 0, 0]), m @ np.array([0, 1.0, 0]), m @ np.array([0, 0, -1.0])


def table(sd):
    """name -> rt_camera, for the scene data `sd` (whose own camera is `own`)."""
    r, u, f = _rotated()
    return {"own": rt.rt_camera.from_buffer_copy(sd.camera),
            "inside": camera((1.5, -1.0, 4.0), r, u, f, 0.6),
            "within": camera((0.3, 0.2, 0.1), (0, 0, 1), (0, 1, 0), (1, 0, 0), 0.9),
            "skew": camera((0.0, 0.5, 6.0), (1.3, 0, 0), (0, 1, 0.2), (0, 0, -1), 0.7),
            "beside": camera((5.5, 0.0, 0.0), (0, 0, -1), (0, 1, 0), (-1, 0, 0), 0.8),
            "far": camera((0.0, 0.0, 40.0), (1, 0, 0), (0, 1, 0), (0, 0, -1), 0.25)}


def swapped(sd, cam):
    return rt.SceneData(sd.positions, sd.texcoords, sd.normals, sd.tangents, sd.material_index, list(sd.materials)[:sd.n_materials],
                        sd.texture_source, sd.images, rt.rt_camera.from_buffer_copy(cam), sd.bg, sd.environment)


def fields(cam):
    """The 13 floats of a camera line of RTAMD_CAMERAS: position, right, up, forward, fov_y."""
    return [*cam.position, *cam.right, *cam.up, *cam.forward, cam.fov_y]
