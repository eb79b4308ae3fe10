#!/usr/bin/env python3
"""Random sequences of the image-space and geometry calls on one warm context against a cold, serial twin:
    image_fuzz.py <first seed> <count>   |   image_fuzz.py --suite   |   image_fuzz.py --replay FILE

plan(seed) is pure numpy (no device, no library): a list of call descriptors, each with its name and arguments, its class and the answer the
call must give ("ok", or refused with a code and the message).  It keeps a ledger of its own to know that answer: the current camera, the
scene generations, the image's camera records, the mark, the hold, whether the pose is stale, the frame number and the ring position
(csrc/hip/pt_image_history.hpp's rules, written a second time; tests/test_image_fuzz_plan.py holds the two against each other).  A plan is one
of two workloads at 48 x 27 (C3: chains through mirror and glass; M5: skin, morph and normals on one pose), moments recorded, on a one-stream
or a devices=[0, 0] context, with 10 to 18 S calls and 0 to 3 D calls between consecutive ones.

S, the calls whose headers say they store into FRAME, T, the ring, the scene or the history:
  render_batch (1-3 frames), burst (2-6 one-frame render_batch_async), reset_frame, next_image, write_back (write_frame + write_moments of an
  earlier result), set_origin, set_rotation (small moves), set_materials (binding 14), set_texture, set_geometry (bindings 3 and 10 of the rest
  pose), reproject_frame, reproject_through, reproject_bilinear, motion_mark, pose_geometry and move_geometry (M5: at a step of the workload,
  preceded by morph_weights and normals_mode; C3: move_geometry of the triangles as they are), reproject_moved, reproject_moved_bilinear,
  history_hold, history_merge, despeckle_frame, filter_for_bloom (a filter call as the producer of the image bloom reads "where the filter
  left it": include/pt_bloom.h).
D, the calls the headers declare read-only, and refused calls:
  read_features, read_features_through and read_through_rays (under two rules), denoise, denoise_guided (1, 3, 5 passes, demodulated or not),
  select_guided, despeckle, fill_frame, tonemap, bloom, bloom_filtered, tonemap_bloom, read_display, read_display_mean, read_display_denoised,
  read_display_denoised_guided, debug_scene_records, pose_triangles (M5: under other matrices); refused_* : one call per family with one bad
  argument (denoise, guided, through, merge, despeckle, tonemap, bloom, reproject, upload, pose).  About a third are marked observed.
  (A D filter call that is not observed leaves another image in the filter's output on the warm context than on the twin, so bloom_filtered
  and tonemap_bloom are only planned while the last filter call ran on both.  pt_debug_scene_records refuses a scene with an upload pending,
  and a D call of the warm context alone may have built it, so debug_scene_records is only planned while the scene is built for sure; a
  multi-stream context refuses it always, and the plan says so.)

run(plan) drives two contexts of the plan's kind in one process:
  warm  every call as written, with no synchronize beyond what the calls do themselves;
  twin  the S calls and the observed D calls only; before each one synchronize() and one refused upload (set_buffer of binding 6, which the
        render path does not consume: pt_set_buffer drops the four record caches before it looks at the binding, and moves no counter:
        DESIGN.md 2.4), after each one synchronize().
After every S call the return value (or the PtError's code and text), read_frame() and read_moments() are compared bit for bit; after every
observed D call everything it returned; at the end every ring image by age, every kind of debug_scene_records, read_features() and
read_features_through().  Every answer on both contexts must be the one the plan predicted.  The twin shares the library, so the end of a
sequence is also held against independent models: on M5 pose.triangles against tests/_normals_model.py's morph_skin_smooth for the last
accepted step, and tonemap() of the final image against tests/_tonemap_model.py.  (The rendered prefix against the oracle is api_fuzz.py's.)

IMAGE_FUZZ_TRACE=<file>: every call is written out before it is made.  IMAGE_FUZZ_SELFTEST=1: one despeckle of the warm context that is not
observed becomes despeckle_frame, and the twin is not told: the next S comparison must fail.  A failing seed's plan is written to
image_fuzz_seed<N>.json under IMAGE_FUZZ_OUT (default: the working directory) for --replay.  Exit code: 0, 1 when a seed failed, and 2 at
once when a call answered with a HIP error or a code the plan did not predict (no further seed is started).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 27
# the suite's seeds (tests/test_image_fuzz_plan.py, tests/test_gpu_image_fuzz.py): of the first 400, sixteen whose plans together meet that test's conditions
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 65, 77, 99, 102, 226, 363)
STEPS = (1, 3, 5, 7)                                              # M5's steps a pose is taken at
ARG, SCENE = -1, -4                                               # PT_ERR_ARG, PT_ERR_SCENE
S_OPS = ("render_batch", "burst", "reset_frame", "next_image", "write_back", "set_origin", "set_rotation", "set_materials", "set_texture", "set_geometry",
         "reproject_frame", "reproject_through", "reproject_bilinear", "motion_mark", "pose_geometry", "move_geometry", "reproject_moved",
         "reproject_moved_bilinear", "history_hold", "history_merge", "despeckle_frame", "filter_for_bloom")
FILTERS = ("denoise", "denoise_guided", "read_display_denoised", "read_display_denoised_guided")
REPROJECTIONS = ("reproject_frame", "reproject_through", "reproject_bilinear", "reproject_moved", "reproject_moved_bilinear")
REFUSED = {"refused_denoise": (ARG, "pt_denoise: iterations must be in [0,8]"),
           "refused_guided": (ARG, "pt_denoise_guided: min_frames must be >= 2"),
           "refused_through": (ARG, "pt_read_features_through: rule.max_depth must be in [0,8]"),
           "refused_merge": (ARG, "pt_history_merge: rule.radius must be in [1,4]"),
           "refused_despeckle": (ARG, "pt_despeckle"),
           "refused_tonemap": (ARG, "pt_tonemap"),
           "refused_bloom": (ARG, "pt_bloom"),
           "refused_reproject": (ARG, "pt_reproject_frame"),
           "refused_upload": (ARG, "pt_set_buffer: binding point not consumed by the render path"),
           "refused_pose": (ARG, "pt_pose_triangles")}
D_OPS = ("read_features", "read_features_through", "read_through_rays", "denoise", "denoise_guided", "select_guided", "despeckle", "fill_frame", "tonemap",
         "bloom", "bloom_filtered", "tonemap_bloom", "read_display", "read_display_mean", "read_display_denoised", "read_display_denoised_guided",
         "debug_scene_records", "pose_triangles") + tuple(REFUSED)
M5_ONLY = ("pose_geometry", "pose_triangles", "refused_pose")
WHO = {"reproject_frame": "pt_reproject_frame", "reproject_through": "pt_reproject_frame_through", "reproject_bilinear": "pt_reproject_frame_bilinear",
       "reproject_moved": "pt_reproject_frame_moved", "reproject_moved_bilinear": "pt_reproject_frame_moved_bilinear"}
THROUGH_RULES = (dict(max_depth=4, min_weight=0.5, lobes=3, key=True), dict(max_depth=2, min_weight=0.9, lobes=1, key=True))
RECORD_KINDS = ("nodes", "nodes80", "tris", "shade", "roots", "ellip", "triObj")
OK = ["ok"]


# ------------------------------------------------------------------------------------------------------------------------ the plan
class Ledger:
    """what the plan knows of a context: pt_image_history.hpp's words, the pose, the frame number, the filter's leftover"""

    def __init__(self):
        self.key = (0, 0)                                         # the current camera: (origin index, rotation index)
        self.scene = self.other = self.writes = 0                 # sceneGen, otherGen, camWrites
        self.cur, self.turned = 0, 0                              # the ring position; pt_next_image calls so far
        self.cam = [None] * 4                                     # per image: (camera key, sceneGen) of a valid camera record
        self.mark = self.hold = None
        self.pose_stale, self.posed = False, None                 # posed: (step, weights' step) of the last accepted pose_geometry
        self.fc = 1                                               # the next frame number
        self.results = 0                                          # S comparisons so far: what write_back can name
        self.dirty = True                                         # an upload since the scene was last built for sure (pt_debug_scene_records refuses then)
        self.left = "none"                                        # the filter's output: none, clean (the last filter call ran on both contexts), dirty

    def written(self):
        self.cam[self.cur] = (self.key, self.scene)
        self.writes += 1
        self.fc = max(self.fc, 2)                                 # (frame 1 stores; the next frames add to what was written)

    def stale_camera(self, who):
        return [ARG, who + ": a scene buffer or texture was uploaded since the image's camera was recorded"]

    def answer(self, op, a):
        """the answer of S call `op`, with the ledger moved on when it is accepted"""
        cam = self.cam[self.cur]
        if op in ("render_batch", "burst"):
            n = len(a["seeds"])
            self.cam[self.cur] = (self.key, self.scene)
            self.writes += 1 if op == "render_batch" else n
            if op == "render_batch":
                self.dirty = False
            self.fc = a["first"] + n
        elif op == "reset_frame":
            self.cam[self.cur] = None; self.writes += 1; self.fc = 1
        elif op == "next_image":
            self.cur = (self.cur + 1) % 4; self.turned += 1
            self.cam[self.cur] = None; self.writes += 1; self.fc = 1
        elif op == "write_back":
            self.written()
        elif op == "set_origin":
            self.key = (a["k"], self.key[1])
        elif op == "set_rotation":
            self.key = (self.key[0], a["k"])
        elif op in ("set_materials", "set_texture"):
            self.scene += 1; self.other += 1; self.dirty = True
        elif op == "set_geometry":
            self.scene += 2; self.pose_stale = True; self.dirty = True
        elif op in ("reproject_frame", "reproject_through", "reproject_bilinear"):
            if cam is None:
                return OK                                         # no camera: nothing to map from
            if cam[1] != self.scene:
                return self.stale_camera(WHO[op])
            self.written()
        elif op == "motion_mark":
            if cam is None:
                return [ARG, "pt_motion_mark: the current image has no camera (render or pt_write_frame first)"]
            if cam[1] != self.scene:
                return self.stale_camera("pt_motion_mark")
            self.mark = (self.cur, self.writes, self.other)
        elif op in ("reproject_moved", "reproject_moved_bilinear"):
            w = WHO[op]
            if op == "reproject_moved_bilinear" and cam is None and self.mark is None:
                return OK
            if self.mark is None:
                return [ARG, w + ": no mark (pt_motion_mark first; a mark serves one call)"]
            if self.mark[0] != self.cur:
                return [ARG, w + ": the mark belongs to another image"]
            if cam is None or self.mark[1] != self.writes:
                return [ARG, w + ": the image's camera is no longer the marked one (a render, pt_write_frame, pt_reset_frame or pt_next_image since the mark)"]
            if self.mark[2] != self.other:
                return [ARG, w + ": binding 5, binding 14 or a texture was uploaded since the mark"]
            self.written(); self.mark = None
        elif op == "history_hold":
            if cam is None:
                return [ARG, "pt_history_hold: the current image has no camera (render or pt_write_frame first)"]
            self.hold = (self.cur, cam[0], self.scene)
        elif op == "history_merge":
            if self.hold is None:
                return [ARG, "pt_history_merge: no hold (pt_history_hold first; a hold serves one merge)"]
            if self.hold[0] != self.cur:
                return [ARG, "pt_history_merge: the hold belongs to another image"]
            if cam is None:
                return [ARG, "pt_history_merge: the image has no camera (pt_reset_frame since the hold)"]
            if cam[0] != self.hold[1]:
                return [ARG, "pt_history_merge: the image's camera no longer has the held frame inputs (a render or pt_write_frame under other inputs)"]
            if self.hold[2] != self.scene:
                return [ARG, "pt_history_merge: a scene buffer or texture was uploaded since the hold"]
            self.written(); self.hold = None
        elif op == "despeckle_frame":
            self.written()
        elif op == "pose_geometry":
            if self.pose_stale:
                return [SCENE, "pt_pose_geometry: the scene was uploaded since pt_pose_create"]
            self.scene += 2; self.posed = (a["step"], a["wstep"]); self.dirty = False
        elif op == "move_geometry":
            self.scene += 2; self.pose_stale = True; self.dirty = False
        elif op == "filter_for_bloom":
            self.left = "clean"
        else:
            raise ValueError(op)
        return OK


def _rule(rs):
    return int(rs.randint(len(THROUGH_RULES)))


def _d_args(rs, op, led, two):
    """(arguments, expected answer) of D call `op`, or None where the ledger cannot tell its answer"""
    a, want = {}, OK
    if op in ("read_features_through", "read_through_rays"):
        a = dict(rule=_rule(rs))
    elif op == "denoise":
        a = dict(iterations=int(rs.choice([1, 3, 5])))
    elif op in ("denoise_guided", "read_display_denoised_guided"):
        a = dict(iterations=int(rs.choice([1, 3, 5])), demod=bool(rs.randint(2)))
    elif op == "read_display_denoised":
        a = dict(iterations=int(rs.choice([1, 3])))
    elif op == "select_guided":
        a = dict(rel_err=float(rs.choice([0.05, 0.2])), demod=bool(rs.randint(2)))
    elif op == "despeckle":
        a = dict(sigmas=float(rs.choice([0.5, 2.0])), radius=int(rs.choice([1, 2])))
    elif op == "fill_frame":
        a = dict(demod=bool(rs.randint(2)))
    elif op == "tonemap":
        a = dict(curve=int(rs.randint(3)), transfer=int(rs.randint(2)))
    elif op == "bloom":
        a = dict(levels=int(rs.randint(1, 7)))
    elif op in ("bloom_filtered", "tonemap_bloom"):
        if led.left == "dirty":
            return None
        a = dict(levels=int(rs.randint(1, 7)))
        if led.left == "none":
            want = [ARG, ("pt_bloom" if op == "bloom_filtered" else "pt_tonemap_bloom") + ": no filtered image on the device"]
    elif op == "read_display":
        a = dict(frames=max(led.fc - 1, 1))
    elif op == "debug_scene_records":
        if led.dirty:
            return None                                           # (a D call of the warm context alone may have built the scene)
        a = dict(kind=str(rs.choice(RECORD_KINDS)))
        if two:
            want = [ARG, "pt_debug_scene_records: a multi-stream context holds one scene per stream"]
    elif op == "pose_triangles":
        a = dict(step=int(rs.choice(STEPS)))
    elif op in REFUSED:
        want = list(REFUSED[op])
    return a, want


def plan(seed):
    """-> {"seed", "workload", "two", "calls": [{"op", "args", "cls", "observed", "want"}], "end"}: see the module's docstring"""
    rs = np.random.RandomState(seed)
    m5 = bool(rs.randint(2))
    out = dict(seed=int(seed), workload="M5" if m5 else "C3", two=bool(rs.randint(2)), calls=[])
    led = Ledger()
    n_s = int(rs.randint(10, 19))
    s_calls = [0]
    queue = []                                                    # S calls a sequence has promised

    def seeds(n):
        return [int(rs.randint(0, 10000)) for _ in range(n)]

    def args_of(op):
        if op == "render_batch":
            return dict(first=led.fc, seeds=seeds(int(rs.randint(1, 4))))
        if op == "burst":
            return dict(first=led.fc, seeds=seeds(int(rs.randint(2, 7))))
        if op == "write_back":
            return dict(result=int(rs.randint(led.results)))
        if op == "set_origin":
            return dict(k=int((led.key[0] + rs.randint(1, 4)) % 4))
        if op == "set_rotation":
            return dict(k=int((led.key[1] + rs.randint(1, 4)) % 4))
        if op == "despeckle_frame":
            return dict(sigmas=float(rs.choice([0.5, 2.0])), radius=int(rs.choice([1, 2])))
        if op in ("pose_geometry", "move_geometry"):
            if not m5:
                return dict(step=0, wstep=0, mode=0)
            return dict(step=int(rs.choice(STEPS)), wstep=int(rs.choice(STEPS)), mode=int(rs.rand() < 0.75))
        if op == "filter_for_bloom":
            return dict(guided=bool(rs.randint(2)), iterations=int(rs.choice([1, 3, 5])), demod=bool(rs.randint(2)))
        if op == "history_merge":
            return dict(radius=int(rs.choice([2, 3])))
        if op in REPROJECTIONS:
            return dict(max_history=float(rs.choice([16.0, 64.0])))
        return {}

    def emit_s(op):
        a = args_of(op)
        want = led.answer(op, a)
        out["calls"].append(dict(op=op, args=a, cls="S", observed=True, want=want))
        led.results += 1
        s_calls[0] += 1

    def emit_d():
        for _ in range(8):
            op = str(rs.choice(D_OPS))
            if op in M5_ONLY and not m5:
                continue
            got = _d_args(rs, op, led, out["two"])
            if got is None:
                continue
            observed = bool(rs.rand() < 1.0 / 3.0)
            if op in FILTERS:
                led.left = "clean" if observed else "dirty"
            out["calls"].append(dict(op=op, args=got[0], cls="D", observed=observed, want=got[1]))
            return

    def refused(op):
        """would S call `op` be refused now?  (asked of a copy of the ledger)"""
        probe = Ledger()
        probe.__dict__.update({k: (list(v) if isinstance(v, list) else v) for k, v in led.__dict__.items()})
        a = dict(step=1, wstep=1, mode=1, k=0, seeds=[0], first=probe.fc)
        return probe.answer(op, a) != OK

    emit_s("reset_frame")
    emit_s("render_batch")                                        # (T is allocated and the image has a camera from here on)
    mover = "pose_geometry" if m5 else "move_geometry"
    while s_calls[0] < n_s:
        if not queue:
            kind = rs.rand()
            if kind < 0.16:                                       # a camera move carried by one of the plain reprojections
                queue = [str(rs.choice(["set_origin", "set_rotation"])), str(rs.choice(["reproject_frame", "reproject_through", "reproject_bilinear"]))]
            elif kind < 0.32:                                     # moved geometry between a mark and its reprojection
                move = mover if rs.rand() < 0.6 else str(rs.choice(["move_geometry", "set_geometry"]))
                queue = ["motion_mark", move, str(rs.choice(["reproject_moved", "reproject_moved_bilinear"]))]
            elif kind < 0.44:                                     # new frames validated against the held history
                queue = ["history_hold", str(rs.choice(["render_batch", "burst"])), "history_merge"]
            else:
                op = str(rs.choice(S_OPS))
                if (op == "pose_geometry" and not m5) or (op == "write_back" and led.results == 0):
                    continue
                if refused(op) and rs.rand() < 0.6:               # most refusals are drawn again: at least 60 % of a plan's S calls are accepted
                    continue
                queue = [op]
        elif rs.rand() < 0.15:                                    # ... and a sequence is sometimes cut into by a call nobody asked for
            op = str(rs.choice(["render_batch", "set_materials", "set_texture", "next_image", "reset_frame", "despeckle_frame", "set_origin"]))
            queue.insert(0, op)
        emit_s(queue.pop(0))
        if s_calls[0] < n_s:
            for _ in range(int(rs.randint(0, 4))):
                emit_d()
    out["end"] = dict(turned=min(led.turned, 3), posed=list(led.posed) if led.posed else None)
    return out


def share_accepted(p):
    s = [c for c in p["calls"] if c["cls"] == "S"]
    return sum(c["want"] == OK for c in s) / len(s)


def history_script(p):
    """the plan as a script of tests/c/image_history_check.cpp, and per script line the index of the plan's call it stands for (None: setup)"""
    lines, of = ["create 32 18", "inputs 1"], [None, None]
    cams = {(0, 0): 1}
    key = [0, 0]

    def add(line, k, n=1):
        for _ in range(n):
            lines.append(line); of.append(k)
    for k, c in enumerate(p["calls"]):
        op, a = c["op"], c["args"]
        if op == "render_batch":
            add("render", k)
        elif op == "burst":
            add("render", k, len(a["seeds"]))
        elif op in ("set_origin", "set_rotation"):
            key[op == "set_rotation"] = a["k"]
            add(f"inputs {cams.setdefault(tuple(key), 5 + len(cams))}", k)
        elif op == "set_geometry":
            add("upload geometry ok", k, 2)
        elif op in ("pose_geometry", "move_geometry"):
            if c["want"] == OK:
                add("move", k)
        elif op in ("read_features", "denoise", "denoise_guided", "select_guided", "despeckle", "fill_frame", "read_display_denoised",
                    "read_display_denoised_guided", "filter_for_bloom"):
            add("records feat cur 0", k)                          # (they ask for the first-hit records under the current inputs)
        elif op in ("read_features_through", "read_through_rays"):
            add(f"records thru cur {a['rule'] + 1}", k)
        else:
            verb = {"reset_frame": "reset", "next_image": "next-image", "write_back": "write", "set_materials": "upload materials ok", "set_texture": "texture",
                    "reproject_frame": "reproject plain", "reproject_through": "reproject through", "reproject_bilinear": "reproject bilinear",
                    "motion_mark": "mark", "reproject_moved": "moved", "reproject_moved_bilinear": "moved-bilinear", "history_hold": "hold",
                    "history_merge": "merge", "despeckle_frame": "despeckle-frame", "refused_upload": "upload other refused"}.get(op)
            if verb:
                add(verb, k)
    return lines, of


# ------------------------------------------------------------------------------------------------------------------------ the run
class Mismatch(Exception):
    def __init__(self, at, why):
        super().__init__(f"call {at}: {why}")
        self.at = at


class DeviceFault(Exception):
    """a HIP error, or a code the plan did not predict"""


def bits(x):
    """anything a call returns, as something == compares bit for bit"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(bits(v) for v in x)
    if isinstance(x, float):
        return np.float64(x).tobytes()
    return x


_M5 = {}


def _m5(scenes):
    """M5 at 48 x 27: the rest workload, the skin, the targets, the ids, and per step (records, weights)"""
    if not _M5:
        rest, bone, weight, targets, X, w, ids, nv = scenes.m5_rippling(1, W, H)
        _M5.update(rest=rest, bone=bone, weight=weight, targets=targets, ids=ids, nv=nv, steps={s: scenes.m5_rippling(s, W, H)[4:6] for s in STEPS}, posed={})
    return _M5


def _m5_triangles(step, wstep, mode):
    """binding 3 of M5 under the records of `step` and the weights of `wstep`, by the models of tests/"""
    import _morph_model as MM
    import _normals_model as NM
    m = _M5
    key = (step, wstep, mode)
    if key not in m["posed"]:
        rest3, X, w = m["rest"].buffers[3], m["steps"][step][0], m["steps"][wstep][1]
        m["posed"][key] = NM.morph_skin_smooth(rest3, m["targets"], w, m["bone"], m["weight"], X, m["ids"]) if mode else \
            MM.morph_skin(rest3, m["targets"], w, m["bone"], m["weight"], X)
    return m["posed"][key]


class Side:
    """one context of a run, with what belongs to it"""

    def __init__(self, name, p, mods, seed):
        renderer, scenes = mods
        self.name, self.p, self.seed, self.R = name, p, seed, renderer
        self.m5 = p["workload"] == "M5"
        self.wl = _m5(scenes)["rest"] if self.m5 else scenes.build("C3", W, H)
        self.r = renderer.Renderer(W, H, devices=[0, 0]) if p["two"] else renderer.Renderer(W, H)
        self.r.load_workload(self.wl)
        self.r.record_moments(True)
        self.buffers = dict(self.wl.buffers)
        self.plan_ = renderer.RefitPlan(self.buffers)
        self.pose = None
        if self.m5:
            m = _M5
            self.pose = self.r.skin_create(m["bone"], m["weight"], 5)
            self.pose.morph_attach(m["targets"])
            self.pose.normals_attach(m["ids"], m["nv"])
        self.results = []
        self.tris = np.array(self.buffers[3], np.float32)         # binding 3 as the context has it (what C3's move_geometry moves to)

    def close(self):
        for x in (self.pose, self.plan_, self.r):
            if x is not None:
                x.close()

    def trace(self, text):
        path = os.environ.get("IMAGE_FUZZ_TRACE")
        if path:
            with open(path, "a") as f:
                f.write(f"seed {self.seed} {self.name}: {text}\n")

    def camera(self, binding, k):
        base = np.asarray(self.wl.buffers[binding], np.float32)
        step = np.array([0.005, 0.0, 0.01], np.float32) if binding == 0 else np.array([0.0, 0.005, 0.0], np.float32)
        return (base + np.float32(k) * step).astype(np.float32)

    def call(self, c, swap=False):
        """-> ("ok", what it returned) or ("refused", code, text)"""
        op = "despeckle_frame" if swap else c["op"]
        self.trace(f"{op} {json.dumps(c['args'], sort_keys=True)}")
        try:
            return ("ok", bits(self.do(op, c["args"])))
        except self.R.PtError as e:
            return ("refused", e.code, str(e).split("] ", 1)[1])

    def guided(self, a):
        return dict(iterations=a["iterations"], albedo_floor=self.R.ALBEDO_FLOOR if a["demod"] else None)

    def do(self, op, a):
        r, R = self.r, self.R
        if op == "render_batch":
            return r.render_batch(a["first"], a["seeds"])
        if op == "burst":
            for k, s in enumerate(a["seeds"]):
                r.render_batch_async(a["first"] + k, [s])
            return None
        if op == "reset_frame":
            return r.reset_frame()
        if op == "next_image":
            return r.next_image()
        if op == "write_back":
            frame, moments = self.results[a["result"]]
            r.write_frame(frame)
            return r.write_moments(moments)
        if op == "set_origin":
            return r.set_buffer(0, self.camera(0, a["k"]))
        if op == "set_rotation":
            return r.set_buffer(1, self.camera(1, a["k"]))
        if op == "set_materials":
            return r.set_buffer(14, self.buffers[14])
        if op == "set_texture":
            return r.set_texture(0, self.wl.sky)
        if op == "set_geometry":
            r.set_buffer(3, self.buffers[3])
            self.tris = np.array(self.buffers[3], np.float32)
            return r.set_buffer(10, self.buffers[10])
        if op == "reproject_frame":
            return r.reproject_frame(max_history=a["max_history"])
        if op == "reproject_through":
            return r.reproject_frame_through(r.through_rule(**THROUGH_RULES[0]), r.reproject_through_rule(max_history=a["max_history"]))
        if op == "reproject_bilinear":
            return r.reproject_frame_bilinear(max_history=a["max_history"])
        if op == "motion_mark":
            return r.motion_mark()
        if op == "reproject_moved":
            return r.reproject_frame_moved(max_history=a["max_history"])
        if op == "reproject_moved_bilinear":
            return r.reproject_frame_moved_bilinear(max_history=a["max_history"])
        if op == "history_hold":
            return r.history_hold()
        if op == "history_merge":
            return r.history_merge(r.validate_rule(radius=a["radius"]))
        if op == "despeckle_frame":
            return r.despeckle_frame(r.despeckle_rule(radius=a["radius"], sigmas=a["sigmas"], min_taps=2))
        if op in ("pose_geometry", "move_geometry"):
            if self.m5:
                X, w = _M5["steps"][a["step"]][0], _M5["steps"][a["wstep"]][1]
                self.pose.morph_weights(w)
                self.pose.normals_mode(a["mode"])
                if op == "pose_geometry":
                    return r.pose_geometry(self.pose, X)
                self.tris = _m5_triangles(a["step"], a["wstep"], a["mode"])
            return r.move_geometry(self.plan_, self.tris)
        if op == "filter_for_bloom":
            return r.denoise_guided(**self.guided(a)) if a["guided"] else r.denoise(a["iterations"])
        # ---- D
        if op == "read_features":
            return r.read_features()
        if op == "read_features_through":
            return r.read_features_through(r.through_rule(**THROUGH_RULES[a["rule"]]))
        if op == "read_through_rays":
            return r.read_through_rays(r.through_rule(**THROUGH_RULES[a["rule"]]))
        if op == "denoise":
            return r.denoise(a["iterations"])
        if op == "denoise_guided":
            return r.denoise_guided(**self.guided(a))
        if op == "select_guided":
            return r.select_guided(a["rel_err"], albedo_floor=R.ALBEDO_FLOOR if a["demod"] else None)
        if op == "despeckle":
            return r.despeckle(r.despeckle_rule(radius=a["radius"], sigmas=a["sigmas"], min_taps=2), want_scale=True)
        if op == "fill_frame":
            return r.fill_frame(albedo_floor=R.ALBEDO_FLOOR if a["demod"] else None)
        if op == "tonemap":
            return r.tonemap(rule=r.tonemap_rule(curve=a["curve"], transfer=a["transfer"]), want_hist=True)
        if op == "bloom":
            return r.bloom(bloom=r.bloom_rule(levels=a["levels"]))
        if op == "bloom_filtered":
            return r.bloom("filtered", bloom=r.bloom_rule(levels=a["levels"]))
        if op == "tonemap_bloom":
            return r.tonemap_bloom("filtered", bloom=r.bloom_rule(levels=a["levels"]), want_hist=True)
        if op == "read_display":
            return r.read_display(a["frames"])
        if op == "read_display_mean":
            return r.read_display_mean()
        if op == "read_display_denoised":
            return r.read_display_denoised(a["iterations"])
        if op == "read_display_denoised_guided":
            return r.read_display_denoised_guided(**self.guided(a))
        if op == "debug_scene_records":
            return r.debug_scene_records(a["kind"])
        if op == "pose_triangles":
            return self.pose.triangles(_M5["steps"][a["step"]][0])
        # ---- refused: one bad argument each
        if op == "refused_denoise":
            return r.denoise(9)
        if op == "refused_guided":
            return r.denoise_guided(min_frames=1)
        if op == "refused_through":
            return r.read_features_through(r.through_rule(max_depth=9, key=True))
        if op == "refused_merge":
            return r.history_merge(r.validate_rule(radius=0))
        if op == "refused_despeckle":
            return r.despeckle(r.despeckle_rule(radius=0))
        if op == "refused_tonemap":
            return r.tonemap(rule=r.tonemap_rule(curve=3))
        if op == "refused_bloom":
            return r.bloom(bloom=r.bloom_rule(levels=0))
        if op == "refused_reproject":
            return r.reproject_frame(depth_tol=-1.0)
        if op == "refused_upload":
            return r.set_buffer(6, np.zeros(4, np.float32))
        if op == "refused_pose":
            return self.pose.triangles(_M5["steps"][1][0][:-1])
        raise ValueError(op)

    def image(self):
        return self.r.read_frame(), self.r.read_moments()

    def ring_image(self, age, torch, shard):
        t = torch.as_tensor(shard._DevArray(self.r.gather_image(age), (H, W, 4)), device=torch.device("cuda", 0))
        self.r.stream_wait()
        return t.cpu().numpy()


def _answered(c, got, at, who):
    """the answer of a call against the plan's prediction"""
    want = c["want"]
    if got[0] == "ok":
        if want != OK:
            raise Mismatch(at, f"{who}: {c['op']} was accepted, the plan says refused {want}")
    else:
        if got[1] == -3:
            raise DeviceFault(f"call {at} ({who}: {c['op']}): HIP error: {got[2]}")
        if want == OK or got[1] != want[0]:
            raise DeviceFault(f"call {at} ({who}: {c['op']}): answered [{got[1]}] {got[2]}, the plan says {want}")
        if not got[2].startswith(want[1]):
            raise Mismatch(at, f"{who}: {c['op']} refused with '{got[2]}', the plan says '{want[1]}'")


def _kept(value):
    """the kept count of a reprojection's return value as bits() has it"""
    return value[0] if isinstance(value, tuple) else value


def run(p, mods=None, counts=None):
    """Run plan `p` on a warm context and its twin.  Raises Mismatch (with .at, the index of the call) or DeviceFault; `counts`, a dict, takes what
    the aggregate conditions of tests/test_gpu_image_fuzz.py ask for."""
    import torch
    if mods is None:
        sys.path.insert(0, ROOT)
        import ptimport
        ptimport.load()
        from pathtracer_0_amd import renderer, scenes
        mods = (renderer, scenes)
    from pathtracer_0_amd import shard
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    counts = {} if counts is None else counts
    selftest = os.environ.get("IMAGE_FUZZ_SELFTEST") == "1"
    swapped = None
    warm = Side("warm", p, mods, p["seed"])
    twin = Side("twin", p, mods, p["seed"])
    sides = (warm, twin)
    try:
        prev = None
        for at, c in enumerate(p["calls"]):
            swap = selftest and swapped is None and c["op"] == "despeckle" and not c["observed"]
            if swap:
                swapped = at
                counts["swapped"] = at
            got = warm.call(c, swap)
            if not swap:
                _answered(c, got, at, "warm")
            if c["cls"] == "S" or c["observed"]:
                twin.r.synchronize()
                try:                                              # the refused upload: drops the twin's four record caches, moves no counter
                    twin.r.set_buffer(6, np.zeros(4, np.float32))
                    raise Mismatch(at, "twin: the upload of binding 6 was accepted")
                except warm.R.PtError as e:
                    if e.code != ARG:
                        raise DeviceFault(f"call {at}: the twin's refused upload answered {e}")
                cold = twin.call(c)
                twin.r.synchronize()
                _answered(c, cold, at, "twin")
                if got != cold:
                    raise Mismatch(at, f"{c['op']}: the warm context returned another value than the twin" if got[0] == cold[0] == "ok" else
                                   f"{c['op']}: warm {got[:2]}, twin {cold[:2]}")
            if c["cls"] == "S":
                before = warm.results[-1] if warm.results else None
                images = [s.image() for s in sides]
                for k, what in enumerate(("FRAME", "T")):
                    if bits(images[0][k]) != bits(images[1][k]):
                        n = int((images[0][k].view(np.uint32) != images[1][k].view(np.uint32)).any(-1).sum())
                        raise Mismatch(at, f"{what} after {c['op']}: {n} pixels differ between the warm context and the twin")
                for s, im in zip(sides, images):
                    s.results.append(im)
                if got[0] == "ok":
                    counts.setdefault("accepted", {}).setdefault(c["op"], 0)
                    counts["accepted"][c["op"]] += 1
                    changed = before is not None and bits(before[0]) != bits(images[0][0])
                    if c["op"] in REPROJECTIONS and 0 < _kept(got[1]) < W * H:
                        counts.setdefault("partly_kept", set()).add(c["op"])
                    if c["op"] in ("history_merge", "despeckle_frame") and changed:
                        counts.setdefault("changed", set()).add(c["op"])
                else:
                    counts.setdefault("refusals", set()).add(got[2].split(": ", 1)[-1][:40])
            elif c["observed"] and c["op"] in FILTERS and prev is not None and prev["op"] != c["op"] and \
                    (prev["op"] in FILTERS or prev["op"] in REPROJECTIONS or prev["op"] == "filter_for_bloom") and prev["want"] == OK:
                counts["filter_after_another"] = counts.get("filter_after_another", 0) + 1
            prev = c
        at = len(p["calls"])
        # ---- the end: the ring, the device records, the feature records
        for age in range(p["end"]["turned"] + 1):
            a, b = (s.ring_image(age, torch, shard) for s in sides)
            if bits(a) != bits(b):
                raise Mismatch(at, f"the ring image of age {age} differs between the warm context and the twin")
        final = [dict(op="read_features", args={}, want=OK), dict(op="read_features_through", args=dict(rule=0), want=OK)] + \
                [dict(op="debug_scene_records", args=dict(kind=k), want=OK) for k in RECORD_KINDS]      # (the scene is built by now on both)
        for c in final:
            a, b = warm.call(c), twin.call(c)
            if a[0] != "ok" and a[1] == -3:
                raise DeviceFault(f"at the end, {c['op']}: {a[2]}")
            if a != b:
                raise Mismatch(at, f"at the end, {c['op']} {c['args']} differs between the warm context and the twin")
        # ---- truth anchors: models that share nothing with the library
        if warm.m5:
            from test_gpu_pose import same_floats
            step, wstep = p["end"]["posed"] or (1, 1)
            for s in sides:
                s.pose.morph_weights(_M5["steps"][wstep][1])
                s.pose.normals_mode(1)
                same_floats(s.pose.triangles(_M5["steps"][step][0]), _m5_triangles(step, wstep, 1), (p["seed"], s.name, "pose.triangles", step, wstep))
        import _tonemap_model as TM
        from test_gpu_tonemap import _same
        col, A = TM.from_frame(warm.r.read_frame())
        rule = TM.rule()
        want = TM.tonemap(col, A, rule, warm.R.tonemap_srgb_thresholds(), W, H)
        for s in sides:
            _same(s.r.tonemap(rule=s.r.tonemap_rule(**rule), want_hist=True), want, (p["seed"], s.name, "tonemap of the final image"))
    finally:
        for s in sides:
            s.close()
    return counts


def one(p, verbose=False):
    try:
        run(p)
    except (Mismatch, DeviceFault, AssertionError) as e:
        out = os.path.join(os.environ.get("IMAGE_FUZZ_OUT", "."), f"image_fuzz_seed{p['seed']}.json")
        with open(out, "w") as f:
            json.dump(p, f, indent=1)
        print(f"seed {p['seed']} {p['workload']} {'two streams' if p['two'] else 'one stream'} {type(e).__name__}: {str(e)[:400]}   (--replay {out})", flush=True)
        if isinstance(e, DeviceFault):
            raise SystemExit(2)                                   # nothing more is started on a device that answered with a fault
        return False
    if verbose:
        print(f"seed {p['seed']} ok {p['workload']} {'two streams' if p['two'] else 'one stream'}: " + "; ".join(c["op"] for c in p["calls"]), flush=True)
    return True


if __name__ == "__main__":
    verbose = os.environ.get("IMAGE_FUZZ_VERBOSE") == "1"
    if sys.argv[1] == "--replay":
        sys.exit(0 if one(json.load(open(sys.argv[2])), verbose=True) else 1)
    todo = SEEDS if sys.argv[1] == "--suite" else range(int(sys.argv[1]), int(sys.argv[1]) + int(sys.argv[2]))
    count = len(todo)
    t0 = time.time()
    bad = sum(0 if one(plan(s), verbose) else 1 for s in todo)
    print(f"{count} sequences, {bad} mismatches / errors, {(time.time() - t0) / count:.2f} s per seed")
    sys.exit(1 if bad else 0)
