"""The spatial-hashing denoiser (linevis_amd/csrc/lv_sh.h) restated with numpy float32 scalars and plain-Python integers, the map as
a dictionary {key word: [sum, count]}.  One hit at a time, no batching and no probing: whatever the order of the hits and wherever a
key lands in its probe window, the map as a set and everything read from it must equal this -- as long as nothing is dropped."""
import ctypes
import ctypes.util
import math
import struct

import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
PROBES = 10
LEVELS = 4
MIN_SAMPLES = 60

# tanf / powf of the C library, as the host code calls them (numpy's float32 tan / power are other implementations)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f, _n in ((_libm.tanf, 1), (_libm.powf, 2)):
    _f.restype = ctypes.c_float
    _f.argtypes = [ctypes.c_float] * _n


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def wang_hash(seed):
    seed &= M32
    seed = (seed ^ 61) ^ (seed >> 16)
    seed = (seed * 9) & M32
    seed = seed ^ (seed >> 4)
    seed = (seed * 0x27d4eb2d) & M32
    seed = seed ^ (seed >> 15)
    return seed


class Params:
    def __init__(self, cam, height, s_p=8.0, s_min_exp=-17, s_nd=3.0, num_cells=10000000):
        self.cam = [F(c) for c in cam]
        self.tan_sp = F(_libm.tanf(F(F(s_p) / F(height))))
        self.s_min = F(_libm.powf(10.0, float(s_min_exp)))
        self.s_nd = F(s_nd)
        self.num_cells = int(num_cells)


def length3(v):
    return np.sqrt(F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def log_step(P, position):
    """floor(log2(s_w / s_min)) as the exponent field of the quotient, or None where the hit is skipped"""
    d = [F(F(p) - c) for p, c in zip(position, P.cam)]
    with np.errstate(all="ignore"):
        quot = F(F(length3(d) * P.tan_sp) / P.s_min)
    e = bits(quot) >> 23
    return None if e == 0 or e >= 255 else e - 127


def cell_size(P, position):
    e = log_step(P, position)
    return None if e is None else F(math.ldexp(float(P.s_min), e))


def normal_words(P, normal):
    n = [F(c) for c in normal]
    d = F(F(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    r = F(F(1.0) / np.sqrt(min(max(d, F(2.0 ** -60)), F(2.0 ** 60))))       # normalize() of the shading code: v * r(v . v)
    return [bits(F(0.0) + F(math.trunc(float(F(F(c * r) * P.s_nd))))) for c in n]


def key_word(P, position, nwords, swd_level):
    s = max(F(swd_level), P.s_min)
    bs = bits(s)
    cx, cy, cz = (bits(np.floor(F(F(p) / s))) for p in position)
    nx, ny, nz = nwords
    h4 = wang_hash(bs + wang_hash(cz + wang_hash(cy + wang_hash(cx))))
    hash_ = wang_hash(nz + wang_hash(ny + wang_hash(nx + h4)))
    c4 = wang_hash(cx + wang_hash(cy + wang_hash(cz + wang_hash(bs))))
    chk = wang_hash(nx + wang_hash(ny + wang_hash(nz + c4)))
    key = (chk << 32) | hash_
    return key if key else 1 << 32


def hit_keys(P, position, normal):
    """the four key words of a hit, or None for a miss / a skipped hit"""
    if all(float(c) == 0.0 for c in normal):
        return None
    swd = cell_size(P, position)
    if swd is None:
        return None
    nw = normal_words(P, normal)
    return [key_word(P, position, nw, F(swd * F(1 << l))) for l in range(LEVELS)]


def quantise(occlusion):
    o = F(occlusion)
    o = F(0.0) if np.isnan(o) else min(max(o, F(0.0)), F(1.0))
    return int(np.floor(F(F(o * F(100.0)) + F(0.5))))


def window(key, num_cells):
    return [(((key & M32) + i) & M32) % num_cells for i in range(PROBES)]


def max_occupied_run(keys, num_cells):
    """Linear probing without deletion fills the same SET of slots in every insertion order.  If that set has no run of PROBES occupied
    slots (around the end of the table too), no key can ever find its window full: dropped == 0 under every schedule.  Returns the
    longest run, or None if sequential insertion itself drops a key."""
    slots = [None] * num_cells
    for k in keys:
        for s in window(k, num_cells):
            if slots[s] is None or slots[s] == k:
                slots[s] = k
                break
        else:
            return None
    occ = [s is not None for s in slots]
    if all(occ):
        return num_cells
    best = run = 0
    for o in occ + occ:
        run = run + 1 if o else 0
        best = max(best, run)
    return best


def denoise(P, cells, noisy, normal_map, position_map):
    """write + read pass of one denoise on (h, w) / (h, w, 4) maps; cells is updated in place.  Returns the read image."""
    h, w = noisy.shape
    keys = {}
    for y in range(h):
        for x in range(w):
            k = hit_keys(P, position_map[y, x, :3], normal_map[y, x, :3])
            if k is not None:
                keys[(y, x)] = k
                q = quantise(noisy[y, x])
                for kw in k:
                    c = cells.setdefault(kw, [0, 0])
                    c[0] += q
                    c[1] += 1
    out = np.zeros((h, w), dtype=np.float32)
    for (y, x), k in keys.items():
        ao, samples = F(0.0), 0
        for kw in k:
            if kw in cells:
                samples += cells[kw][1]
                ao = F(ao + F(F(cells[kw][0]) / F(100.0)))
            if samples >= MIN_SAMPLES:
                break
        out[y, x] = F(ao / F(samples)) if samples > 0 else F(0.0)
    return out


def cells_as_set(cells):
    return {(k, v[0], v[1]) for k, v in cells.items()}


def given_maps(width=24, height=16):
    """The hand-built maps of the GPU tests: rows 0 .. 6 a plane a millimetre in front of CAMERAS[0] whose pixels lie 2e-4 apart (cells
    of a few pixels that do not line up with the normals' blocks, so the a-trous tail has neighbours with the same normal and another
    value to blend), rows 7 .. 8 misses, rows 9 .. 15 a sloped plane whose distance to the camera spans more than two octaves; normals
    in all eight octants, in blocks of three columns; occlusion values that include 0, 1 and ties of the quantisation."""
    rng = np.random.RandomState(11)
    normal = np.zeros((height, width, 4), dtype=np.float32)
    position = np.zeros((height, width, 4), dtype=np.float32)
    noisy = rng.rand(height, width).astype(np.float32)
    noisy[0, :6] = [0.0, 1.0, 0.005, 0.015, 0.995, 0.125]
    for y in range(height):
        for x in range(width):
            if y in (7, 8):
                continue
            o = (x // 3) % 8
            n = np.array([1.0 if o & 1 else -1.0, 2.0 if o & 2 else -2.0, 3.0 if o & 4 else -3.0])
            normal[y, x, :3] = n / np.linalg.norm(n)
            if y < 7:
                position[y, x, :3] = (0.05 + 2e-4 * (x - 12), 2e-4 * (y - 3), 0.799)
            else:
                position[y, x, :3] = (-0.9 + 0.15 * x, 0.1 * (y - 12), -0.2 - 0.2 * x)
            position[y, x, 3] = 1.0
    return noisy, normal, position


CAMERAS = ((0.05, 0.0, 0.8), (0.3, -0.2, 1.7))
