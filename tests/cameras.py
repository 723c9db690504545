"""The camera family of the general-camera tests (test_cameras.py on the CPU, test_gpu_cameras.py on the GPU): named cameras as plain
data, applied to a common.Case through camera.look_at / camera.perspective.  The data sets of the suite are normalised into
[-0.25, 0.25]^3 (scenes.normalize), which is what the distances below refer to.

lv_set_camera takes two arbitrary 4 x 4 matrices; what the rest of the suite passes is default_camera with a moving eye.  Every entry
here leaves that slice in one direction: roll, target, field of view, near / far, lens shift (proj[8], proj[9]), pixel aspect."""
import numpy as np

from linevis_amd import camera


def _deg(a):
    return float(np.float32(np.deg2rad(a)))


def _rolled_up(angle_deg, tilt=0.0):
    """(0, 1, 0) turned by angle_deg about z, with a z component `tilt` (look_at orthogonalises it against the viewing direction)"""
    a = np.deg2rad(angle_deg)
    return (float(-np.sin(a)), float(np.cos(a)), float(tilt))


DEFAULTS = dict(target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=camera.DEFAULT_FOVY, near=camera.DEFAULT_NEAR, far=camera.DEFAULT_FAR,
                shift=(0.0, 0.0), pixel_aspect=1.0)

CAMERAS = {
    # the reference's fixed test camera: what every other test of the suite uses
    "default": dict(eye=camera.DEFAULT_POSITION),
    # rolled by 37 degrees, the eye off the z axis: no entry of the view matrix's rotation is zero
    "roll37": dict(eye=(0.3, 0.2, 0.7), up=_rolled_up(37.0)),
    # the target is not the origin: the data set sits off-centre
    "target_off": dict(eye=(0.1, 0.05, 0.8), target=(0.2, -0.15, 0.1)),
    # fovy 15 degrees from distance 2.5 with a tilted up vector: hit distances ~2.5 (the textbook roots lose digits)
    "narrow_far": dict(eye=(1.2, 0.8, 2.04), up=_rolled_up(-20.0, 0.3), fovy=_deg(15.0)),
    # fovy 120 degrees from distance 0.35: the projected radius of a tube grows by 1 / cos(off-axis angle) towards the corners
    "wide_close": dict(eye=(0.05, -0.03, 0.35), fovy=_deg(120.0)),
    # straight down the y axis: the default up vector would be parallel to the viewing direction
    "straight_down": dict(eye=(0.0, 0.8, 0.0), up=(0.0, 0.0, -1.0)),
    # near / far = 0.6 / 0.95 cut the data set (view-space depths of the default eye: 0.55 .. 1.05)
    "tight_clip": dict(eye=(0.0, 0.0, 0.8), near=0.6, far=0.95),
    # the eye inside the data set, rolled, fovy 90 degrees, near 0.001: segments straddle the camera plane
    "inside_rolled": dict(eye=(0.03, -0.02, 0.05), target=(-0.2, 0.1, -0.3), up=_rolled_up(25.0), fovy=_deg(90.0), near=0.001),
    # lens shift (an off-centre frustum, what tiled and stereo embedders pass): proj[8], proj[9] != 0
    "lens_shift": dict(eye=(0.0, 0.0, 0.8), shift=(0.35, -0.2)),
    # one quadrant of a frame rendered as 2 x 2 tiles from close by: half the tangent range, ndc shifted by a whole unit -- the centre
    # of the full frame (the optical axis) is a corner of this viewport, so the projected radius does not grow away from its middle
    "tiled_quadrant": dict(eye=(0.05, 0.03, 0.4), fovy=float(np.float32(2.0 * np.arctan(0.25))), shift=(1.0, -1.0)),
    # near / far = 0.001 / 10000: the worst conditioned projection of the family
    "huge_range": dict(eye=(0.0, 0.0, 0.8), near=0.001, far=10000.0),
    # non-square pixels: the projection's aspect is not width / height
    "nonsquare_pixels": dict(eye=(0.1, 0.1, 0.8), pixel_aspect=1.6),
    # rolled, looking away from the origin from inside the data set's box: a part of the data set is behind the camera
    "away_rolled": dict(eye=(0.05, 0.0, 0.1), target=(0.45, 0.25, -0.6), up=_rolled_up(-50.0, 0.2), fovy=_deg(75.0)),
}
NAMES = sorted(CAMERAS)
# cameras whose eye lies inside the data set's bounding box: some segment has one end behind the camera plane
INSIDE = ("inside_rolled", "away_rolled")
# where the conservative screen bound of the sharded PPLL's cull pass is least certain
CULL_CRITICAL = ("wide_close", "roll37", "lens_shift", "tiled_quadrant", "nonsquare_pixels")

# viewports: wide, tall, and one whose sides are multiples neither of 8 nor of the PPLL tile (2 x 8)
VIEWPORTS = {"wide": (72, 48), "tall": (40, 88), "ragged": (93, 61)}


def get(name):
    cam = dict(DEFAULTS)
    cam.update(CAMERAS[name])
    return cam


def matrices(cam, width, height):
    """(view, proj, fovy, near, far) of a camera description for a width x height viewport, float32 column-major like default_camera"""
    cam = dict(DEFAULTS, **cam)
    view = camera.look_at(cam["eye"], cam["target"], cam["up"])
    proj = camera.perspective(cam["fovy"], float(width) / float(height) * float(cam["pixel_aspect"]), cam["near"], cam["far"])
    proj[8], proj[9] = np.float32(cam["shift"][0]), np.float32(cam["shift"][1])   # column 2, rows 0 and 1: ndc = proj[0] x / -z - shift
    return view, proj, float(cam["fovy"]), float(cam["near"]), float(cam["far"])


def apply_camera(case, cam):
    """Sets case.view / proj / fovy / near / far from a camera description (or the name of one); returns the case."""
    if isinstance(cam, str):
        cam = get(cam)
    case.view, case.proj, case.fovy, case.near, case.far = matrices(cam, case.width, case.height)
    return case


def view_space_z(case, positions):
    """float64 view-space z of world positions under the case's view matrix"""
    v = np.asarray(case.view, np.float64).reshape(4, 4).T
    return np.asarray(positions, np.float64) @ v[2, :3] + v[2, 3]


def segments_straddling_the_camera_plane(case):
    """number of segments with one line point in front of the camera plane and one behind it"""
    z = view_space_z(case, case.points["linePosition"])
    a, b = z[case.seg[:, 0]], z[case.seg[:, 1]]
    return int(((a < 0) != (b < 0)).sum())
