"""numpy restatement of the tracker step (include/bevf.h, bevf_track_step_f32; csrc/track.hip) and the fixed scenes
the host and GPU tests share.

`step` is an explicit Python loop over streams, detections and tracks.  Association distances are fp64 (the kernel's are fp32 squared
distances: `margins` records how far every decisive comparison is from flipping, and tests/test_tracking_host.py::test_scene_margins
keeps that >= 1e-3 in every scene, so both decide alike).  What is stored is rounded to float32 exactly where the kernel rounds:
Python floats are IEEE doubles and Python never fuses a multiply with an add, so every stored column but the coasted yaw (atan2) is the
kernel's bit for bit.  The reference project has no tracker; the host tests pin this file with closed forms instead."""
import math

import numpy as np

STATE = (("track_box", np.float32, (7,)), ("track_vel", np.float32, (2,)), ("track_score", np.float32, ()),
         ("track_label", np.int64, ()), ("track_id", np.int64, ()), ("track_age", np.int32, ()), ("track_hits", np.int32, ()))


def new_state(B: int, T: int) -> dict:
    st = {name: np.zeros((B, T) + tail, dtype) for name, dtype, tail in STATE}
    st["track_id"][:] = -1
    st["track_count"] = np.zeros(B, np.int32)
    st["next_id"] = np.zeros(B, np.int64)
    return st


def _f32(v: float) -> float:
    """Round a double to float32, returned as the (exact) double."""
    return float(np.float32(v))


def step(st: dict, boxes, vels, scores, labels, count, ego, dt, max_dist, max_age: int, birth_score: float, class_aware: bool,
         margins: list = None) -> dict:
    """Advance `st` in place by one frame; returns det_track_id / det_hits / det_slot (B,N) and overflow (B,).  margins (a list) gets
    ('dist', |best - max_dist|), ('rival' | 'second', second - best: the runner-up inside | outside the limit; 'tie' when they are
    equal) and ('score', |score - birth_score|) for every decisive comparison."""
    B, N = boxes.shape[:2]
    T = st["track_box"].shape[1]
    C = len(max_dist)
    out = {"det_track_id": np.full((B, N), -1, np.int64), "det_hits": np.zeros((B, N), np.int32),
           "det_slot": np.full((B, N), -1, np.int32), "overflow": np.zeros(B, np.int32)}
    birth32 = float(np.float32(birth_score))
    for b in range(B):
        n, tc = min(max(int(count[b]), 0), N), min(max(int(st["track_count"][b]), 0), T)
        m = [[float(ego[b, r, c]) for c in range(4)] for r in range(3)]
        d = float(dt[b])
        tbox, tvel, tscore = st["track_box"][b].copy(), st["track_vel"][b].copy(), st["track_score"][b].copy()
        tlab, tid, tage, thits = st["track_label"][b].copy(), st["track_id"][b].copy(), st["track_age"][b].copy(), st["track_hits"][b].copy()
        taken, det_of = [False] * tc, [-1] * tc
        match = [-1] * n                                             # old slot, -1 unmatched, -2 invalid
        # 1. association
        for i in range(n):
            x, y, z = (float(v) for v in boxes[b, i, :3])
            vx, vy = (float(v) for v in vels[b, i])
            if not all(math.isfinite(v) for v in (x, y, z, vx, vy, float(scores[b, i]))):
                match[i] = -2
                continue
            px, py = x - vx * d, y - vy * d
            qx = _f32(((m[0][0] * px + m[0][1] * py) + m[0][2] * z) + m[0][3])
            qy = _f32(((m[1][0] * px + m[1][1] * py) + m[1][2] * z) + m[1][3])
            lab = int(labels[b, i])
            md = float(max_dist[lab if 0 <= lab < C else 0])
            best, best_d, second_d = -1, math.inf, math.inf
            for s in range(tc):
                if taken[s] or (class_aware and int(tlab[s]) != lab):
                    continue
                dx, dy = qx - float(tbox[s, 0]), qy - float(tbox[s, 1])
                dist = math.sqrt(dx * dx + dy * dy)
                if dist < best_d:                                    # strict: a tie stays with the lower slot; NaN never wins
                    best, best_d, second_d = s, dist, best_d
                elif dist < second_d:
                    second_d = dist
            if best >= 0 and margins is not None:
                margins.append(("dist", abs(best_d - md)))
                if best_d <= md and second_d < math.inf:               # rival: the runner-up is inside the limit too
                    kind = "tie" if second_d == best_d else ("rival" if second_d <= md else "second")
                    margins.append((kind, second_d - best_d))
            if best >= 0 and md >= 0.0 and best_d <= md:
                taken[best], det_of[best], match[i] = True, i, best
        # 2. / 3. / 5. old tracks
        new = new_state(1, T)
        pos = 0
        yaw_step = math.atan2(m[1][0], m[0][0])
        for s in range(tc):
            if taken[s]:
                i = det_of[s]
                new["track_box"][0, pos], new["track_vel"][0, pos], new["track_score"][0, pos] = boxes[b, i], vels[b, i], scores[b, i]
                new["track_age"][0, pos], new["track_hits"][0, pos] = 0, thits[s] + 1
                out["det_track_id"][b, i], out["det_hits"][b, i], out["det_slot"][b, i] = tid[s], thits[s] + 1, pos
            else:
                if int(tage[s]) + 1 > max_age:
                    continue
                p = [float(v) for v in tbox[s, :3]]
                vx, vy = float(tvel[s, 0]), float(tvel[s, 1])
                ux, uy, uz = p[0] - m[0][3], p[1] - m[1][3], p[2] - m[2][3]
                wx, wy = m[0][0] * vx + m[1][0] * vy, m[0][1] * vx + m[1][1] * vy
                box = tbox[s].copy()
                box[0] = np.float32(((m[0][0] * ux + m[1][0] * uy) + m[2][0] * uz) + wx * d)
                box[1] = np.float32(((m[0][1] * ux + m[1][1] * uy) + m[2][1] * uz) + wy * d)
                box[2] = np.float32((m[0][2] * ux + m[1][2] * uy) + m[2][2] * uz)
                box[6] = np.float32(float(tbox[s, 6]) - yaw_step)
                new["track_box"][0, pos], new["track_vel"][0, pos] = box, (np.float32(wx), np.float32(wy))
                new["track_score"][0, pos] = tscore[s]
                new["track_age"][0, pos], new["track_hits"][0, pos] = tage[s] + 1, thits[s]
            new["track_label"][0, pos], new["track_id"][0, pos] = tlab[s], tid[s]
            pos += 1
        # 4. births
        next_id = int(st["next_id"][b])
        for i in range(n):
            if match[i] != -1:
                continue
            sc = float(scores[b, i])
            if margins is not None:
                margins.append(("score", abs(sc - birth32)))
            if not sc >= birth32:
                continue
            if pos >= T:
                out["overflow"][b] += 1
                continue
            new["track_box"][0, pos], new["track_vel"][0, pos], new["track_score"][0, pos] = boxes[b, i], vels[b, i], scores[b, i]
            new["track_label"][0, pos], new["track_id"][0, pos] = labels[b, i], next_id
            new["track_age"][0, pos], new["track_hits"][0, pos] = 0, 1
            out["det_track_id"][b, i], out["det_hits"][b, i], out["det_slot"][b, i] = next_id, 1, pos
            next_id += 1
            pos += 1
        for name, _, _ in STATE:
            st[name][b] = new[name][0]
        st["track_count"][b], st["next_id"][b] = pos, next_id
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
# A scene = dict(name, T, C, max_dist [C], max_age, birth_score, class_aware, init (a state or None), frames [dict(boxes, velocities,
# scores, labels, count, ego_motion, dt)]).  Objects sit on a 17 x 17 lattice of 6 m cells (+-48 m), move at most 1.5 m per step and
# are detected within 0.05 m, and the distance limits stay between 0.5 m and 2.5 m unless a case says otherwise: the nearest wrong
# track is metres away, the right one centimetres.

GRID, CELL = 17, 6.0
EDGE_COUNTS = (0, 1, 63, 64, 65, 257)


def cell_xy(c: int):
    return ((c % GRID) - GRID // 2) * CELL, ((c // GRID) - GRID // 2) * CELL


def rigid(yaw: float, tx: float, ty: float, tz: float = 0.0) -> np.ndarray:
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw)
    m[:3, 3] = tx, ty, tz
    return m


def frame(B: int, N: int) -> dict:
    return {"boxes": np.zeros((B, N, 7), np.float32), "velocities": np.zeros((B, N, 2), np.float32), "scores": np.zeros((B, N), np.float32),
            "labels": np.zeros((B, N), np.int64), "count": np.zeros(B, np.int32), "ego_motion": np.tile(np.eye(4), (B, 1, 1)),
            "dt": np.full(B, 0.5, np.float32)}


def put(fr: dict, b: int, xy, vel=(0.0, 0.0), score=0.5, label=0, z=-1.0, yaw=0.3) -> int:
    """Append one detection to stream b of fr; returns its row."""
    i = int(fr["count"][b])
    fr["boxes"][b, i] = (xy[0], xy[1], z, 1.9, 4.5, 1.6, yaw)
    fr["velocities"][b, i], fr["scores"][b, i], fr["labels"][b, i] = vel, score, label
    fr["count"][b] = i + 1
    return i


def seed_tracks(st: dict, b: int, cells, rng, C: int, age: int = 0) -> None:
    """Tracks on `cells` of stream b, as births of an earlier frame would have left them (ids 100, 101, ...)."""
    for s, c in enumerate(cells):
        x, y = cell_xy(c)
        st["track_box"][b, s] = (x + rng.uniform(-1, 1), y + rng.uniform(-1, 1), rng.uniform(-2, 0), 1.9, 4.5, 1.6, rng.uniform(-3, 3))
        st["track_vel"][b, s] = rng.uniform(-3, 3, 2)
        st["track_score"][b, s], st["track_label"][b, s] = rng.uniform(0.2, 0.9), c % C
        st["track_id"][b, s], st["track_age"][b, s], st["track_hits"][b, s] = 100 + s, age, 1 + s % 5
    st["track_count"][b], st["next_id"][b] = len(cells), 100 + len(cells)


def detect(fr: dict, b: int, st: dict, s: int, rng, ego=None, score=None, label=None, noise=0.05) -> int:
    """A detection of track s of stream b one step later: the track moved by its velocity, seen from the new frame (ego: current ->
    previous, None = identity)."""
    M = np.eye(4) if ego is None else ego
    dtb = float(fr["dt"][b])
    p = st["track_box"][b, s, :3].astype(np.float64)
    v = np.array([st["track_vel"][b, s, 0], st["track_vel"][b, s, 1], 0.0], np.float64)
    cur = M[:3, :3].T @ (p + v * dtb - M[:3, 3])
    vcur = M[:3, :3].T @ v
    xy = cur[:2] + rng.uniform(-noise, noise, 2) / math.sqrt(2.0)
    return put(fr, b, xy, vcur[:2], rng.uniform(0.3, 0.9) if score is None else score,
               int(st["track_label"][b, s]) if label is None else label, z=cur[2],
               yaw=float(st["track_box"][b, s, 6]) - math.atan2(M[1, 0], M[0, 0]))


def _scene(name, T, C, frames, init=None, max_dist=2.0, max_age=3, birth_score=0.1, class_aware=True) -> dict:
    md = np.full(C, max_dist, np.float32) if np.isscalar(max_dist) else np.asarray(max_dist, np.float32)
    return {"name": name, "T": T, "C": C, "max_dist": md, "max_age": max_age, "birth_score": birth_score, "class_aware": class_aware,
            "init": init, "frames": frames}


def edge_scene(tcnt: int, ndet: int, pad: int = 3) -> dict:
    """One step from tcnt tracks with ndet detections: detection j looks at lattice cell 7 j mod 289 (all distinct); a cell below tcnt
    holds a track, which the detection matches, the others are births.  `pad` rows past count hold NaN and huge values."""
    rng = np.random.default_rng(1000 * tcnt + ndet)
    T, C = (300 if tcnt > 256 else 96), 3
    st = new_state(1, T)
    seed_tracks(st, 0, range(tcnt), rng, C)
    N = ndet + (pad if ndet else 0)
    fr = frame(1, N)
    for j in range(ndet):
        c = (7 * j) % (GRID * GRID)
        score = 0.9 - 0.8 * j / max(ndet, 1)
        if c < tcnt:
            detect(fr, 0, st, c, rng, score=score)
        else:
            x, y = cell_xy(c)
            put(fr, 0, (x + rng.uniform(-1, 1), y + rng.uniform(-1, 1)), rng.uniform(-3, 3, 2), score, c % C)
    if N > ndet:
        fr["boxes"][0, ndet:], fr["velocities"][0, ndet:], fr["scores"][0, ndet:] = np.nan, 3e38, np.inf
        fr["boxes"][0, ndet, :2], fr["labels"][0, ndet:] = st["track_box"][0, 0, :2], -7          # a padding row right on a track
    return _scene(f"edge_t{tcnt}_n{ndet}", T, C, [fr], st)


def rule_scenes() -> list:
    """One small scene per rule of the step (names say which)."""
    out = []
    rng = np.random.default_rng(7)
    C = 3

    def base(tcnt=6, T=16, B=1, age=0):
        st = new_state(B, T)
        for b in range(B):
            seed_tracks(st, b, range(b, b + tcnt), rng, C, age)
        return st

    st = base()                                                       # no detections: every track coasts, under a rotating ego
    fr = frame(1, 4)
    fr["ego_motion"][0] = rigid(0.2, 1.5, -0.4, 0.1)
    out.append(_scene("all_coast", 16, C, [fr], st))

    fr = frame(1, 5)                                                  # an empty state: every detection is born
    for j in range(5):
        put(fr, 0, cell_xy(20 + j), (1.0, -0.5), 0.8 - 0.1 * j, j % C)
    out.append(_scene("all_born", 16, C, [fr], None))

    st = base()                                                       # every track matched
    fr = frame(1, 6)
    for s in (3, 0, 5, 1, 4, 2):
        detect(fr, 0, st, s, rng)
    out.append(_scene("all_matched", 16, C, [fr], st))

    st = base()                                                       # nothing matched: detections 3 m from the tracks' projections
    fr = frame(1, 6)
    for s in range(6):
        i = detect(fr, 0, st, s, rng)
        fr["boxes"][0, i, 0] += 3.0
    out.append(_scene("none_matched", 16, C, [fr], st))

    st = base(tcnt=6, T=8)                                            # full state: 6 coast, 2 born, 3 overflow and take no id
    fr = frame(1, 5)
    for j in range(5):
        put(fr, 0, cell_xy(40 + j), (0.0, 0.0), 0.8 - 0.1 * j, 0)
    fr2 = frame(1, 2)                                                 # next frame: the next births would continue the ids, none fits
    put(fr2, 0, cell_xy(60), (0.0, 0.0), 0.8, 0)
    out.append(_scene("overflow", 8, C, [fr, fr2], st))

    for age, name in ((1, "age_at_max_survives"), (2, "age_past_max_drops")):     # max_age = 2: age 1 -> 2 stays, 2 -> 3 goes
        st = base(age=age)
        fr = frame(1, 2)
        detect(fr, 0, st, 2, rng)
        out.append(_scene(name, 16, C, [fr], st, max_age=2))

    st = base()                                                       # the right place, the wrong class: born beside the coasting track
    fr = frame(1, 2)
    detect(fr, 0, st, 1, rng, label=(int(st["track_label"][0, 1]) + 1) % C)
    detect(fr, 0, st, 4, rng)
    out.append(_scene("class_mismatch", 16, C, [fr], st))
    out.append(_scene("class_agnostic", 16, C, [fr], {k: v.copy() for k, v in st.items()}, class_aware=False))

    st = base()                                                       # per-class limits: 0.7 m off matches class 1 (1 m), not class 0 (0.5 m)
    fr = frame(1, 6)
    for s in range(6):
        i = detect(fr, 0, st, s, rng, noise=0.0)
        fr["boxes"][0, i, 1] += 0.7
    out.append(_scene("per_class_max_dist", 16, C, [fr], st, max_dist=[0.5, 1.0, 2.5]))

    st = base()                                                       # dt = 0: detections where the tracks are, velocities ignored
    fr = frame(1, 6)
    fr["dt"][:] = 0.0
    for s in range(6):
        detect(fr, 0, st, s, rng)
    out.append(_scene("dt_zero", 16, C, [fr], st))

    fr = frame(1, 4)                                                  # scores 2e-3 either side of birth_score = 0.25
    for j, sc in enumerate((0.252, 0.248, 0.9, 0.1)):
        put(fr, 0, cell_xy(80 + j), (0.0, 0.0), sc, 0)
    out.append(_scene("birth_score_sides", 16, C, [fr], None, birth_score=0.25))

    st = base()                                                       # NaN / inf detections inside count: no match, no birth
    fr = frame(1, 8)
    for s in range(6):
        detect(fr, 0, st, s, rng)
    put(fr, 0, cell_xy(90), (0.0, 0.0), 0.7, 0)
    fr["boxes"][0, 1, 0], fr["velocities"][0, 3, 1], fr["scores"][0, 4], fr["boxes"][0, 6, 2] = np.nan, np.inf, np.nan, -np.inf
    out.append(_scene("nan_detection", 16, C, [fr], st))

    st = base(tcnt=5, B=3)                                            # three streams, different counts and ego motions, one launch
    fr = frame(3, 7)
    fr["ego_motion"][1], fr["ego_motion"][2] = rigid(-0.1, 0.8, 0.3), rigid(0.4, -2.0, 1.0, -0.2)
    fr["dt"][:] = (0.5, 0.25, 0.1)
    for s in (0, 2, 4):
        detect(fr, 0, st, s, rng, fr["ego_motion"][0])
    for s in range(5):
        detect(fr, 2, st, s, rng, fr["ego_motion"][2])
    put(fr, 2, cell_xy(100), (1.0, 1.0), 0.6, 1)
    put(fr, 2, cell_xy(101), (1.0, 1.0), 0.05, 1)                     # below birth_score
    out.append(_scene("three_streams", 16, C, [fr], st))

    st = base()                                                       # labels outside [0, C) use max_dist[0] and still match by label
    st["track_label"][0, 2] = 9
    fr = frame(1, 2)
    detect(fr, 0, st, 2, rng)
    put(fr, 0, cell_xy(110), (0.0, 0.0), 0.6, -4)
    out.append(_scene("label_out_of_range", 16, C, [fr], st, max_dist=[1.0, 0.01, 0.01]))
    return out


def sequence_scene(frames: int = 12, B: int = 2, K: int = 9, seed: int = 3, ego: bool = True, T: int = 32, max_age: int = 3,
                   dropouts=((1, 3, 1), (2, 5, 3), (4, 4, 4), (7, 8, 2)), clutter: bool = True) -> dict:
    """K <= 9 objects per stream, 30 m apart, on constant world velocities of at most 1.5 m/s per axis, seen from an ego that drives
    and turns; dropouts = (object, first frame, length) detection gaps; one clutter detection per frame, 6 m from the last one, far
    from the objects.  Ground truth: frames[f]['truth'][b][row] = object, -1 for clutter."""
    rng = np.random.default_rng(seed)
    C = 3
    pos = np.zeros((B, K, 2))
    vel = rng.uniform(-1.5, 1.5, (B, K, 2))
    for b in range(B):
        for k in range(K):
            pos[b, k] = (30.0 * (k % 3 - 1) + 2.0 * b, 30.0 * (k // 3 - 1) - 1.0 * b)
    pose = [np.eye(4) for _ in range(B)]                              # ego -> world
    out = []
    for f in range(frames):
        fr = frame(B, K + 2)
        fr["truth"] = [[] for _ in range(B)]
        for b in range(B):
            new_pose = pose[b] @ rigid(0.06 * (b + 1), 2.0, 0.1 * b) if (ego and f) else pose[b]
            fr["ego_motion"][b] = np.linalg.inv(pose[b]) @ new_pose   # current -> previous (temporal.ego_motion)
            pose[b] = new_pose
            inv = np.linalg.inv(pose[b])
            order = rng.permutation(K)
            for rank, k in enumerate(order):
                if any(o == k and f0 <= f < f0 + ln for o, f0, ln in dropouts):
                    continue
                w = np.array([*(pos[b, k] + vel[b, k] * 0.5 * f), -1.0, 1.0])
                c = inv @ w
                v = inv[:3, :3] @ np.array([*vel[b, k], 0.0])
                put(fr, b, c[:2] + rng.uniform(-0.03, 0.03, 2), v[:2], 0.9 - 0.05 * rank, int(k % C), z=c[2])
                fr["truth"][b].append(int(k))
            if clutter:
                put(fr, b, (-70.0 + 6.0 * f, 95.0), (0.0, 0.0), 0.3, int(f % C))
                fr["truth"][b].append(-1)
        out.append(fr)
    return _scene(f"sequence_{'ego' if ego else 'still'}", T, C, out, None, max_dist=2.0, max_age=max_age)


RIVAL_T = (96, 300)                                                   # the 4- and the 16-slots-per-lane kernel
TIE_SLOTS = ((2, 7), (20, 84))                                        # two lanes; one lane (slots s and s + 64)


def _move(st: dict, s: int, base: int, dx: float, dy: float) -> None:
    """Track s of stream 0 to (dx, dy) from track `base`, with its label: a rival of `base`."""
    st["track_box"][0, s, :2] = st["track_box"][0, base, :2] + np.array([dx, dy], np.float32)
    st["track_label"][0, s] = st["track_label"][0, base]


def _near(fr: dict, st: dict, base: int, dx: float, dy: float, score: float) -> int:
    """A standing detection (dx, dy) from track `base` of stream 0, with its label."""
    x, y = (float(v) for v in st["track_box"][0, base, :2])
    return put(fr, 0, (x + dx, y + dy), (0.0, 0.0), score, int(st["track_label"][0, base]))


def rival_scene(T: int) -> dict:
    """Detections with 2 to 4 free tracks of their label inside max_dist = 2 m (ids are 100 + slot; detections stand still, so q is
    the detection's centre).  In order:
      rows 0-2  tracks 1, 4, 2 in three lanes: row 0 is 0.3 m from 4 and 0.7 m from 1 (the nearest is the higher slot), row 1 then takes
                the runner-up 1 with 2 still in reach, row 2 takes 2;
      rows 3-4  tracks 10 and 74 in one lane: row 3 is 0.2 m from 74 and 0.6 m from 10, row 4 takes 10;
      row 5     tracks 12 and 76 in one lane, the lower slot the nearer;
      row 6     four rivals, 20, 84 and (T = 300: 148, else 22) around 21's neighbour 20: 84 is the nearest, 0.08 m before 20."""
    rng = np.random.default_rng(50 + T)
    C, tcnt = 3, (200 if T > 256 else 90)
    st = new_state(1, T)
    seed_tracks(st, 0, range(tcnt), rng, C)
    third = 148 if tcnt > 148 else 22
    for s, base, dx, dy in ((4, 1, 1.0, 0.0), (2, 1, 0.0, 1.5), (74, 10, 0.8, 0.0), (76, 12, 0.8, 0.0), (84, 20, 0.9, 0.0),
                            (third, 20, 0.0, 0.9), (21, 20, -0.9, 0.0)):
        _move(st, s, base, dx, dy)
    fr = frame(1, 9)
    for j, (base, dx, dy) in enumerate(((1, 0.7, 0.0), (1, 0.6, 0.1), (1, 0.2, 0.9), (10, 0.6, 0.0), (10, 0.1, 0.1), (12, 0.1, 0.0),
                                        (20, 0.5, 0.3))):
        _near(fr, st, base, dx, dy, 0.9 - 0.05 * j)
    return _scene(f"rivals_T{T}", T, C, [fr], st)


def tie_scene(T: int) -> dict:
    """Exact ties.  Tracks 2 and 7 (two lanes) stand 2 m apart on integer coordinates and row 0 stands exactly between them, 1 m from
    each: the lower slot, 2, takes it; tracks 20 and 84 (one lane) likewise with row 1.  Row 2, 0.5 m beside row 0, then gets 7.
    Every coordinate is an integer or a half, the velocities are 0 and the ego stands: q, the differences and d2 = 1 are exact in
    fp32 and in fp64, so both arithmetics see the same tie (test_scene_margins checks the coordinates)."""
    rng = np.random.default_rng(60 + T)
    C = 3
    st = new_state(1, T)
    seed_tracks(st, 0, range(90), rng, C)
    fr = frame(1, 4)
    for j, (lo, hi) in enumerate(TIE_SLOTS):
        x, y = cell_xy(lo)
        st["track_box"][0, lo, :2], st["track_box"][0, hi, :2] = (x, y), (x + 2.0, y)
        st["track_label"][0, hi] = st["track_label"][0, lo]
        put(fr, 0, (x + 1.0, y), (0.0, 0.0), 0.9 - 0.1 * j, int(st["track_label"][0, lo]))
    x, y = cell_xy(TIE_SLOTS[0][0])
    put(fr, 0, (x + 1.0, y + 0.5), (0.0, 0.0), 0.5, int(st["track_label"][0, TIE_SLOTS[0][0]]))
    return _scene(f"tie_T{T}", T, C, [fr], st)


def rival_scenes() -> list:
    return [rival_scene(T) for T in RIVAL_T] + [tie_scene(T) for T in RIVAL_T]


def all_scenes() -> list:
    """Every fixed scene of tests/test_gpu_tracking.py."""
    edges = [edge_scene(t, n) for t in EDGE_COUNTS for n in EDGE_COUNTS]
    return edges + rule_scenes() + rival_scenes() + [sequence_scene()]


def run(scene: dict, margins: list = None):
    """The restatement over a scene: [(outputs, state copy)] per frame."""
    B = scene["frames"][0]["boxes"].shape[0]
    st = new_state(B, scene["T"]) if scene["init"] is None else {k: v.copy() for k, v in scene["init"].items()}
    res = []
    for fr in scene["frames"]:
        o = step(st, fr["boxes"], fr["velocities"], fr["scores"], fr["labels"], fr["count"], fr["ego_motion"], fr["dt"], scene["max_dist"],
                 scene["max_age"], scene["birth_score"], scene["class_aware"], margins)
        res.append((o, {k: v.copy() for k, v in st.items()}))
    return res
