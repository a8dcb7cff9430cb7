"""One long-lived context driven through TF, option, isosurface and stream changes -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_state_cases.py (CPU: the script is not vacuous) and tests/test_gpu_state.py (GPU:
one context per kind held to the references through the whole chain), so they cannot drift apart.
Importing this module needs neither a GPU nor libvr.so.

The chain is CHAIN: eight transfer functions, each an "epoch" of rendering.  An epoch's script
(round) is a list of ops in the order the context sees them:

    ("iso", (value, rgb))       set_isosurface
    ("opt", (field, value))     set_options with one render field changed
    ("step", Step)              one frame (delivery "batch": the three views) rendered and checked

The five modes come in a seeded order (the first mode of epoch e is a seeded permutation's entry
e mod 5, so every mode is the first one after a TF change); between two modes the isosurface moves on
and two option fields change: the next of a seeded order of all fields, and the next of the fields
the coming mode reads (and, ahead of VRC under the default TF, axis_columns goes to 2: the column
path's gate is then seen open before and after the TFs that shut it).  Steps carry a delivery and a
stream, both dealt round-robin from a seeded start.  The step after an "async_pair" step is the pair's second frame: queued on the same stream
behind the first, whatever lies between them in the script, and both are read after one synchronize.
"""
import functools

import numpy as np

import param_cases as pc
from param_cases import ISO_RGB, Case
from test_dvr_ref import seeded_tf
from test_gpu_parity import _tf_n

E, T = 1, 2   # vr_api.h VR_FLAG_ESS, VR_FLAG_ERT
SEED = 5

CAL = 255.0
FRAME_A = (48, 36, 64)
# Past the TEST march's plane-table cutoff.  launch_test_march takes the table while
#     lds + 16 KB <= 32 KB,   lds = round16(16 n_tf + occupancy bytes under ESS) + 16 (S + 2 K) [+ 4 (d1 + d2 + d3) at test_corners 3]
# with K = 4 and, for blob() -- 5 x 5 x 4 cells of 8^3 voxels, 4 words -- 16 occupancy bytes.  Under the
# default TF (the only one of at most 4 intervals and class 0 = TF(0), which the table needs) that is
# 16 (S + 8) <= 16384 - 80, S <= 1011 (1012 without ESS; 985 at test_corners 3).  1100 is past all three.
FRAME_B = (40, 30, 1100)
PLANE_TABLE_MAX_S = (16384 - 80) // 16 - 8
assert PLANE_TABLE_MAX_S == 1011 and FRAME_A[2] <= 985 and FRAME_B[2] > 1012

VIEW_NAMES = ("z", "x_back", "obl")
MODE_NAMES = ("vrc", "test", "dvr", "mip", "iso")
FLAGS_A = (0, E, T, E | T)
FLAGS_B = (0, E | T)
FRAME_B_MODES = ("test", "dvr")

DELIVERIES = ("host", "async_pair", "batch", "tiles")
GROUP_DELIVERIES = ("host", "async_pair", "batch")   # what a multi-GPU context supports
STREAMS = ("own", "caller1", "caller2")

OPAQUE0 = [(0.0, 1.0, (0.1, 0.2, 0.3, 0.05)), (0.3, 0.6, (0.9, 0.5, 0.1, 0.4))]
ZERO_IS_ONE = [(0.3, 0.6, (0.9, 0.8, 0.7, 0.4)), (0.0, 0.05, (0.0, 0.0, 0.0, 0.0)),
               (0.05, 0.3, (0.2, 0.5, 0.3, 0.2))]   # test_nonzero_class_of_zero's
ALL_CLEAR = [(0.0, 0.5, (0.8, 0.1, 0.3, 0.0)), (0.5, 1.0, (0.2, 0.7, 0.9, 0.0))]

CHAIN = ("default", "ten", "opaque0", "zero_is_one", "seeded17", "all_clear", "seeded256", "default")


@functools.lru_cache(maxsize=None)
def tf_of(name):
    return {"default": pc.default_tf, "ten": lambda: _tf_n(10), "opaque0": lambda: list(OPAQUE0),
            "zero_is_one": lambda: list(ZERO_IS_ONE), "seeded17": lambda: seeded_tf(17, 17),
            "all_clear": lambda: list(ALL_CLEAR), "seeded256": lambda: seeded_tf(256, 256)}[name]()


ISO_CYCLE = ((128.0, ISO_RGB), (-1.0, ISO_RGB), (40.0, (0.2, 0.9, 0.4)))
ISO_AT_CREATE = (0.5 * CAL, (1.0, 1.0, 1.0))   # vr_create: half of cal_max, white

# render options (vr_set_options may change them): field -> its values in the order the script visits
# them, the default first
OPTION_VALUES = {
    "batch": (0, 8, 16),
    "cull": (2, 0, 1),
    "axis_columns": (1, 2, 0),
    "view_table_reuse": (1, 0),
    "axis_table": (1, 0),
    "occ_lds": (1, 0),
    "leaf_map_pad": (1, 0),
    "exact_skip": (1, 0),
    "test_plane_march": (1, 0),
    "run_words": (0, 1, 2),
    "table_split": (1, 0),
    "frames_in_flight": (1, 2, 3, 0),
    "column_overlap": (1, 0),
}
# the modes whose frames a field can change the path of (vr_api.cpp: make_vrc_march, make_test,
# launch_frame, visible_rect, frames_in_flight)
READERS = {
    "batch": ("vrc",), "axis_columns": ("vrc",), "view_table_reuse": ("vrc",), "axis_table": ("vrc",),
    "leaf_map_pad": ("vrc",), "exact_skip": ("vrc",), "run_words": ("vrc",), "table_split": ("vrc",),
    "column_overlap": ("vrc",),
    "occ_lds": ("vrc", "test", "dvr"),
    "test_plane_march": ("test",),
    "cull": MODE_NAMES, "frames_in_flight": MODE_NAMES,
}
assert set(READERS) == set(OPTION_VALUES)


class Step:
    """One rendered frame of the script (delivery "batch": the three views, `view` names none of them)."""

    def __init__(self, epoch, mode, view, flags, frame):
        self.epoch, self.mode, self.view, self.flags, self.frame = epoch, mode, view, flags, frame
        self.delivery = self.stream = None
        self.second = False    # the second frame of the async pair the step before it opened
        self.index = -1        # among the epoch's steps

    def views(self):
        return VIEW_NAMES if self.delivery == "batch" else (self.view,)

    def __repr__(self):
        return (f"Step(epoch {self.epoch} {CHAIN[self.epoch]} #{self.index} {self.mode} {self.view} flags {self.flags} "
                f"frame {self.frame} {self.delivery}{' (second)' if self.second else ''} stream {self.stream})")


@functools.lru_cache(maxsize=None)
def script(seed=SEED, deliveries=DELIVERIES):
    """The whole chain's ops, one tuple per epoch (option values depend on the epochs before)."""
    rng = np.random.default_rng(seed)
    first_modes = [MODE_NAMES[i] for i in rng.permutation(len(MODE_NAMES))]
    all_fields = [sorted(OPTION_VALUES)[i] for i in rng.permutation(len(OPTION_VALUES))]
    read_by = {m: [f for f in all_fields[::-1] if m in READERS[f]] for m in MODE_NAMES}
    turn = {f: 0 for f in OPTION_VALUES}
    n_all, n_read, n_iso = 0, {m: 0 for m in MODE_NAMES}, 0
    d_i, s_i = int(rng.integers(len(deliveries))), int(rng.integers(len(STREAMS)))
    rounds = []
    for epoch in range(len(CHAIN)):
        first = first_modes[epoch % len(MODE_NAMES)]
        rest = [m for m in MODE_NAMES if m != first]
        order = [first] + [rest[i] for i in rng.permutation(len(rest))]
        ops, steps = [], []
        for k, mode in enumerate(order):
            if k:   # between the modes of the round
                ops.append(("iso", ISO_CYCLE[n_iso % len(ISO_CYCLE)]))
                n_iso += 1
                picks = [all_fields[n_all % len(all_fields)], read_by[mode][n_read[mode] % len(read_by[mode])]]
                n_all += 1
                n_read[mode] += 1
                for f in dict.fromkeys(picks):
                    turn[f] += 1
                    ops.append(("opt", (f, OPTION_VALUES[f][turn[f] % len(OPTION_VALUES[f])])))
                # the one pick that is not the seed's: ahead of VRC under the default TF the column path is
                # forced, so that its gate is seen open in the first epoch and again after it was shut
                f = "axis_columns"
                if mode == "vrc" and CHAIN[epoch] == "default" and OPTION_VALUES[f][turn[f] % 3] != 2:
                    while OPTION_VALUES[f][turn[f] % 3] != 2:
                        turn[f] += 1
                    ops.append(("opt", (f, 2)))
            mine = [Step(epoch, mode, v, fl, FRAME_A) for v in VIEW_NAMES for fl in FLAGS_A]
            if mode in FRAME_B_MODES:
                mine += [Step(epoch, mode, "obl", fl, FRAME_B) for fl in FLAGS_B]
            for i in rng.permutation(len(mine)):
                steps.append(mine[i])
                ops.append(("step", mine[i]))
        for i, st in enumerate(steps):
            st.index = i
            if i and steps[i - 1].delivery == "async_pair" and not steps[i - 1].second:
                st.delivery, st.stream, st.second = "async_pair", steps[i - 1].stream, True
                continue
            st.delivery, st.stream = deliveries[d_i % len(deliveries)], STREAMS[s_i % len(STREAMS)]
            d_i += 1
            s_i += 1
            if st.delivery == "async_pair" and i == len(steps) - 1:   # no frame left to pair it with
                st.delivery = "host"
        rounds.append(tuple(ops))
    return tuple(rounds)


def round(epoch, seed=SEED, deliveries=DELIVERIES):   # noqa: A001 (the issue's name for an epoch's script)
    """The seeded list of ops of one epoch."""
    return script(seed, deliveries)[epoch]


def bits_of(n_tf):
    """(class bits of the VRC class volume, bits per voxel of TEST's corner volume) of a TF of n_tf intervals."""
    cb = 2 if n_tf <= 4 else (4 if n_tf <= 16 else 8)
    return cb, 8 * cb


def class_of_zero(tf):
    """(class, alpha) of the value 0 through the oracle's TF scan."""
    otf = pc.oracle.tf_array(tf)
    k = pc.oracle.tf_class(otf[0], otf[1], 0.0)
    return k, float(tf[k][2][3])


def occupied(tf):
    """Some voxel value of blob() (k / 255, k = 0 .. 255) has a class of non-zero alpha."""
    otf = pc.oracle.tf_array(tf)
    return any(tf[pc.oracle.tf_class(otf[0], otf[1], float(np.float32(k) / np.float32(CAL)))][2][3] != 0.0
               for k in range(256))


_REFS = {}


def reference(name):
    """The Reference of blob() under a TF of the chain, one per TF and process."""
    if name == "default":
        return pc.shared_reference("blob")
    if name not in _REFS:
        _REFS[name] = pc.Reference(pc.blob(), CAL, tf=tf_of(name))
    return _REFS[name]


class Model:
    """What the context should hold after the ops so far: TF, isosurface, render options."""

    def __init__(self):
        self.epoch = 0
        self.tf_name = CHAIN[0]
        self.iso = ISO_AT_CREATE
        self.options = {f: v[0] for f, v in OPTION_VALUES.items()}
        self.last_mutation = ("create",)

    def set_epoch(self, epoch):
        self.epoch, self.tf_name = epoch, CHAIN[epoch]
        self.last_mutation = ("tf", self.tf_name)

    def apply(self, op):
        kind, arg = op
        if kind == "iso":
            self.iso = arg
        elif kind == "opt":
            self.options[arg[0]] = arg[1]
        else:
            raise ValueError(kind)
        self.last_mutation = op

    @property
    def tf(self):
        return tf_of(self.tf_name)

    @property
    def n_tf(self):
        return len(self.tf)

    @property
    def zero_transparent(self):
        return class_of_zero(self.tf)[1] == 0.0

    def case(self, step, view):
        kw = {"iso": self.iso[0], "rgb": self.iso[1]} if step.mode == "iso" else {}
        return Case(view, pc.MODES[step.mode], frame=step.frame, **kw)

    def expected(self, step, view):
        """The reference's exact frame of a step's view under the current state (MIP and ISO: no TF)."""
        ref = reference("default" if step.mode in ("mip", "iso") else self.tf_name)
        return ref.frame(self.case(step, view))

    def columns(self, step, view, one_gpu_32bit=True):
        """Whether the step's whole-frame render takes the column path: True / False where the gate is
        decided by the state alone, None where it is the auto ratio's (axis_columns = 1).  (axis_table = 0
        switches the axis views' march off, and the column path is a variant of it.)"""
        if step.mode != "vrc" or not self.zero_transparent or self.options["axis_columns"] == 0 or \
                self.options["axis_table"] == 0 or view not in pc.AXIS_VIEWS or not one_gpu_32bit:
            return False
        return True if self.options["axis_columns"] == 2 else None

    def what(self, step, view=None):
        return (f"epoch {step.epoch} tf {self.tf_name} mode {step.mode} view {view or step.view} flags {step.flags} "
                f"frame {step.frame} delivery {step.delivery}{'/second' if step.second else ''} stream {step.stream} "
                f"step #{step.index} iso {self.iso} last mutation {self.last_mutation}")
