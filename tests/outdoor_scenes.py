"""Deterministic outdoor lidar scans for the tests (test-side only: pure numpy, nothing from loam_amd).

The synthetic room of loam_amd/csrc/synth.h is 20 x 16 x 6 m with a ceiling: every beam returns, every range is under
15 m, and the plane index picks 0.5 m cells. The scenes here are shaped like the reference's own use (64- or 128-beam
sensors outdoors, LidarParams(H, W, 1.0, 120.0)): feature sets over 100-250 m, larger index cells, dense 3x3x3 blocks,
no-return beams and returns beyond max_range.

A scan is H scan lines x W azimuth steps, row-major [line][column], line 0 the lowest beam, azimuth 2*pi*c/W, points in
the sensor frame as float64 (H*W, 3); a beam that hits nothing within 200 m returns (0, 0, 0). The world is the ground
plane z = 0 and axis-aligned boxes; the sensor rides 1.8 m above the ground. Poses are 7-vectors [qx qy qz qw tx ty tz].
"""
import numpy as np

MAX_HIT = 200.0
SENSOR_HEIGHT = 1.8
SCENES = ("canyon", "lot", "field")
# elevation fan (top, bottom) in degrees: a 64 / 128-beam sensor with its fan tilted down; the field's is symmetric
FANS = {"canyon": (2.0, -24.8), "lot": (2.0, -24.8), "field": (15.0, -15.0)}


def _box(x0, x1, y0, y1, z0, z1):
    return np.array([[x0, y0, z0], [x1, y1, z1]], dtype=np.float64)


def scene_boxes(name, seed):
    """the boxes of a scene (list of (2, 3) arrays: low corner, high corner), world frame"""
    rng = np.random.default_rng([{"canyon": 1, "lot": 2, "field": 3}[name], seed])
    boxes = []
    if name == "canyon":
        # a street: building fronts at y = +-12 m from x = -60 to 60 m, open ground beyond both ends
        for s in (-1.0, 1.0):
            x = -60.0
            while x < 60.0:  # fronts of differing height and setback
                w = min(rng.uniform(8.0, 20.0), 60.0 - x)
                y0 = 12.0 + rng.uniform(0.0, 1.5)
                boxes.append(_box(x, x + w, *sorted((s * y0, s * (y0 + 6.0))), 0.0, rng.uniform(8.0, 25.0)))
                x += w
        for _ in range(8):  # parked cars and kiosks on both sides of the lane the sensor drives along
            cx, cy = rng.uniform(-55.0, 55.0), rng.choice([-1.0, 1.0]) * rng.uniform(5.0, 10.0)
            lx, ly, lz = rng.uniform(3.0, 5.0), rng.uniform(1.6, 2.2), rng.uniform(1.3, 2.6)
            boxes.append(_box(cx - lx / 2, cx + lx / 2, cy - ly / 2, cy + ly / 2, 0.0, lz))
        for s in (-1.0, 1.0):  # lamp posts along both kerbs (edge features that pin the pose along the street)
            for x in np.arange(-54.0, 55.0, 12.0) + rng.uniform(-2.0, 2.0):
                boxes.append(_box(x - 0.15, x + 0.15, s * 10.5 - 0.15, s * 10.5 + 0.15, 0.0, 6.0))
    elif name == "lot":
        # a walled lot, walls at +-80 m with two gates each (the ground beyond them is open), boxes and poles inside
        for axis in (0, 1):
            for s in (-1.0, 1.0):
                gates = np.sort(rng.uniform(-60.0, 60.0, 2))
                cuts = [-80.5, gates[0] - 6.0, gates[0] + 6.0, gates[1] - 6.0, gates[1] + 6.0, 80.5]
                for a, b in zip(cuts[0::2], cuts[1::2]):
                    if b <= a:
                        continue
                    lo, hi = sorted((s * 80.0, s * 80.5))
                    boxes.append(_box(a, b, lo, hi, 0.0, 8.0) if axis == 0 else _box(lo, hi, a, b, 0.0, 8.0))
        while len(boxes) < 8 + 60:
            cx, cy = rng.uniform(-72.0, 72.0, 2)
            if abs(cx) < 8.0 and abs(cy) < 8.0:
                continue  # (the sensor stands near the middle)
            if rng.random() < 0.35:  # pole
                r, h = rng.uniform(0.15, 0.4), rng.uniform(4.0, 7.0)
                boxes.append(_box(cx - r, cx + r, cy - r, cy + r, 0.0, h))
            else:
                lx, ly, h = rng.uniform(2.0, 9.0), rng.uniform(2.0, 9.0), rng.uniform(1.2, 4.5)
                boxes.append(_box(cx - lx / 2, cx + lx / 2, cy - ly / 2, cy + ly / 2, 0.0, h))
    elif name == "field":
        # open ground: a few low objects, all at least 15 m away and in a few azimuth clusters (empty sectors)
        centres = rng.uniform(0.0, 2 * np.pi, 3)
        for _ in range(40):
            az = centres[rng.integers(3)] + rng.normal() * 0.3
            r = rng.uniform(15.0, 110.0)
            cx, cy = r * np.cos(az), r * np.sin(az)
            lx, ly, h = rng.uniform(1.0, 6.0), rng.uniform(1.0, 6.0), rng.uniform(1.0, 4.0)
            boxes.append(_box(cx - lx / 2, cx + lx / 2, cy - ly / 2, cy + ly / 2, 0.0, h))
    else:
        raise ValueError(name)
    return boxes


def beam_directions(H, W, fan):
    """unit ray directions in the sensor frame, (H*W, 3), row-major [line][column]"""
    top, bottom = fan
    el = np.radians(bottom + (top - bottom) * np.arange(H) / (H - 1))
    az = 2.0 * np.pi * np.arange(W) / W
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    d = np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], np.broadcast_to(se, (H, W))], axis=-1)
    return d.reshape(-1, 3)


def _rz(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def cast(boxes, origin, yaw, H, W, fan, sigma, rng):
    """one scan from a sensor at `origin` (world) with heading `yaw` (rad); range noise sigma * N(0, 1)"""
    d_sensor = beam_directions(H, W, fan)
    d = (d_sensor @ _rz(yaw).T).reshape(H, W, 3)
    o = np.asarray(origin, dtype=np.float64)
    t = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = -o[2] / d[..., 2]
        t = np.where((d[..., 2] < 0.0) & (tg > 0.0), tg, t)  # ground
        inv = 1.0 / d
        for b in boxes:
            cols = _columns_facing(b, o, yaw, W)
            t1, t2 = (b[0] - o) * inv[:, cols], (b[1] - o) * inv[:, cols]
            near = np.nanmax(np.minimum(t1, t2), axis=-1)
            far = np.nanmin(np.maximum(t1, t2), axis=-1)
            tc = t[:, cols]
            t[:, cols] = np.where((near <= far) & (near > 0.0) & (near < tc), near, tc)
    t = t.reshape(-1)
    hit = t <= MAX_HIT
    r = np.where(hit, t + sigma * rng.standard_normal(len(t)), 0.0)
    return np.ascontiguousarray(d_sensor * r[:, None])


def _columns_facing(b, o, yaw, W):
    """the azimuth columns whose rays can meet box b (all of them if the sensor stands above its footprint)"""
    if b[0, 0] <= o[0] <= b[1, 0] and b[0, 1] <= o[1] <= b[1, 1]:
        return np.arange(W)
    a = np.array([np.arctan2(y - o[1], x - o[0]) for x in b[:, 0] for y in b[:, 1]]) - yaw
    a = a[0] + np.angle(np.exp(1j * (a - a[0])))  # (unwrapped around the first corner: the box spans less than pi)
    c0, c1 = int(np.floor(a.min() * W / (2 * np.pi))) - 1, int(np.ceil(a.max() * W / (2 * np.pi))) + 1
    return np.arange(c0, c1 + 1) % W


def yaw_pose(yaw, t):
    """pose7 of a rotation about z by `yaw` followed by translation t"""
    return np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2), *t], dtype=np.float64)


def sensor_origin(name, seed):
    """(world position, heading) of a pair's target scan"""
    rng = np.random.default_rng([11, {"canyon": 1, "lot": 2, "field": 3}[name], seed])
    if name == "canyon":
        xy = (rng.uniform(-25.0, 25.0), rng.uniform(-1.5, 1.5))
    elif name == "lot":
        xy = tuple(rng.uniform(-4.0, 4.0, 2))
    else:
        xy = tuple(rng.uniform(-5.0, 5.0, 2))
    return np.array([xy[0], xy[1], SENSOR_HEIGHT]), rng.uniform(-0.1, 0.1) + (0.0 if name == "canyon" else rng.uniform(-np.pi, np.pi))


def scan_at(name, scene_seed, origin, yaw, H=64, W=1024, sigma=0.01, noise_seed=0):
    return cast(scene_boxes(name, scene_seed), origin, yaw, H, W, FANS[name], sigma, np.random.default_rng(noise_seed))


def pair(name, seed, H=64, W=1024, sigma=0.01, scene_seed=0):
    """(target scan, source scan, target_T_source): the source sensor has moved 0.3-1.5 m forward and turned by up to 2
    degrees. For the scan-pair entry points the pair is laid out target scan first (np.stack((target, source)))."""
    boxes = scene_boxes(name, scene_seed)
    o, yaw = sensor_origin(name, seed)
    rng = np.random.default_rng([23, {"canyon": 1, "lot": 2, "field": 3}[name], seed])
    fwd, dyaw = rng.uniform(0.3, 1.5), np.radians(rng.uniform(-2.0, 2.0))
    motion = yaw_pose(dyaw, (fwd, 0.0, 0.0))  # in the target sensor's frame
    o_src = o + _rz(yaw) @ np.array([fwd, 0.0, 0.0])
    tgt = cast(boxes, o, yaw, H, W, FANS[name], sigma, np.random.default_rng([31, seed, 0]))
    src = cast(boxes, o_src, yaw + dyaw, H, W, FANS[name], sigma, np.random.default_rng([31, seed, 1]))
    return tgt, src, motion


def to_world(scan, origin, yaw):
    """sensor-frame points of a scan taken at (origin, yaw) in the world frame"""
    return np.ascontiguousarray(scan @ _rz(yaw).T + np.asarray(origin))
