"""The scenes the tests of the RGBA camera gradient share (test_rgba_camera.py, test_gpu_rgba_camera.py): the
volume of test_rgba.py's _scene (seed 3, rounded to float32), one upstream gradient per image size, and four cases -- a thin
volume at rate 1 under the default pose; an opaque one at rate 2 with jitter under a panned, rolled, zoomed pose (rays that
terminate early); a camera inside the box; and a max_samples clip."""
import math

import numpy as np

from test_rgba import _scene as _rgba_scene

F32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
LOOK_FROM = (2.2, 1.1, 1.7)
POSED = dict(look_at=(0.2, -0.1, 0.15), up=(0.3, 1.0, -0.2), fov_rad=math.radians(24.0))

CASES = {
    "default_sr1": dict(vshape=(10, 9, 11), opaque=False, WH=(12, 10), sr=1.0, S=512, seed=0),
    "posed_sr2_ert_jit": dict(vshape=(10, 9, 11), opaque=True, WH=(12, 10), sr=2.0, S=512, seed=77, **POSED),
    "inside": dict(vshape=(12, 12, 12), opaque=True, WH=(9, 9), sr=1.0, S=512, seed=5, look_from=(0.3, 0.2, 0.4),
                   look_at=(-0.5, 0.1, -0.6), fov_rad=math.radians(35.0)),
    "clip_S6": dict(vshape=(10, 9, 11), opaque=False, WH=(12, 10), sr=2.0, S=6, seed=0, look_at=(0.1, 0.0, 0.0)),
}


def volume(vshape=(10, 9, 11), opaque=False):
    return F32(_rgba_scene(vshape=vshape, WH=(2, 2), seed=3, opaque=opaque)["vol"])


def make(vshape=(10, 9, 11), opaque=False, WH=(12, 10), sr=1.0, S=512, seed=0, view=0, look_from=LOOK_FROM, **pose):
    """The input dict of rgba_pose_reference.run_case, rounded to what the kernels read."""
    inp = dict(vol=volume(vshape, opaque), look_from=F32(look_from), grad_out=F32(np.random.RandomState(1).standard_normal((*WH, 4))),
               sr=np.float64(sr), max_samples=np.int32(S), jitter_seed=np.int64(seed), view=np.int32(view))
    inp.update({k: F32(v) for k, v in pose.items()})
    return inp


def case(name, **over):
    return make(**dict(CASES[name], **over))
