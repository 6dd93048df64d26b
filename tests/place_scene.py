"""The recognition scene of the place stage (test infrastructure, not a test file): `places` windows along one
wide texture, `fillers` frames of another texture, then the places again in reverse order, each disturbed by a small shift,
rotation and scale.  Nearest-neighbour views, as tests/test_gpu_track.py renders them."""
import numpy as np

from test_gpu_track import _view, _warp

FULL = dict(W=320, H=240, places=12, fillers=4, step=160, cap=2048, min_gap=4)
# cut down for the GPU: the last place's revisit follows it after the two fillers, three frames on
REDUCED = dict(W=160, H=120, places=6, fillers=2, step=80, cap=256, min_gap=3)


def _window(scene, ox, oy, W, H, G=None):
    """The W x H view whose origin is scene pixel (ox, oy), seen through the view-to-view map G."""
    Hs, Ws = scene.shape[:2]
    T = np.array([[1, 0, ox - (Ws - W) / 2], [0, 1, oy - (Hs - H) / 2], [0, 0, 1.0]])  # _view centres its window
    return _view(scene, T @ (G if G is not None else np.eye(3)), W, H)


def frames(oracle, W, H, places, fillers, step, **_):
    """(frames uint8 (2 places + fillers, H, W, 4), twin: {revisit frame: the frame of the place it shows})."""
    texture = oracle.synth_frame(15 * step, 400, 300)
    other = oracle.synth_frame(15 * step // 2, 400, 77)
    rng = np.random.default_rng(1)
    out = [_window(texture, 40 + step * i, 60, W, H) for i in range(places)]
    out += [_window(other, 40 + step // 2 * i, 60, W, H) for i in range(fillers)]
    twin = {}
    for i in reversed(range(places)):
        dx, dy = rng.uniform(-10, 10, 2)
        angle = rng.uniform(-4, 4)
        scale = rng.uniform(0.97, 1.03)
        twin[len(out)] = i
        out.append(_window(texture, 40 + step * i, 60, W, H, _warp(dx, dy, scale, angle, W=W, H=H)))
    return np.stack(out), twin


def place_of(g, places, fillers, **_):
    """The place frame g shows; None for a filler."""
    if g < places:
        return g
    return None if g < places + fillers else 2 * places + fillers - 1 - g
