"""The tracer recorder (gpe_tracers_*, include/gpe.h) restated over tests/_oracle_model.OracleModel.  TEST
INFRASTRUCTURE ONLY.

The definition, with nothing of the implementation in it: step one at a time; after every step that leaves
steps_seen % every == 0 (and at every sample()) look each tracked uid up in the model's uid array and copy that
particle's pos, prev and storage index -- quiet NaN and UID_ABSENT when no particle carries the uid or uids are off.
The ring keeps the newest `frames` frames; read() delivers the newest min(count, capacity), oldest first.
"""
import collections

import numpy as np

F32 = np.float32
UID_ABSENT = 0xFFFFFFFF
TRACERS_MAX = 65536
Frames = collections.namedtuple("Frames", "step pos prev index count recorded")


def frame_of(uids, pos, prev, tracked):
    """One frame: (pos f32[k,2], prev f32[k,2], index u32[k]) of the particles whose uid is tracked[j]; uids None = off."""
    k = len(tracked)
    fp = np.full((k, 2), np.nan, F32)
    fq = np.full((k, 2), np.nan, F32)
    fi = np.full(k, UID_ABSENT, np.uint32)
    if uids is not None and len(uids):
        order = np.argsort(uids, kind="stable")
        at = np.searchsorted(uids[order], tracked)
        at[at == len(order)] = 0
        found = uids[order[at]] == tracked
        who = order[at[found]]
        fp[found], fq[found], fi[found] = pos[who], prev[who], who.astype(np.uint32)
    return fp, fq, fi


class TracerModel:
    """Wraps an OracleModel: drive the steps through step() / run() here -- or step the model itself and call after_step()
    after each step, as tests/_interactive_sequences.py does -- and everything else on the model itself."""

    def __init__(self, model, uids, every=1, frames=1024):
        self.m = model
        self.tracked = np.array(uids, np.uint32).reshape(-1)
        assert 1 <= len(self.tracked) <= TRACERS_MAX and len(np.unique(self.tracked)) == len(self.tracked)
        assert every >= 1 and frames >= 1 and model.uids is not None
        self.every, self.frames = int(every), int(frames)
        self.steps_seen = 0
        self.recorded = 0
        self.ring = collections.deque(maxlen=self.frames)      # (step, pos, prev, index), oldest first

    def sample(self):
        m = self.m
        if m._sim is not None:                                 # mid-run: the Sim holds the arrays
            pos, prev = m._sim.pos, m._sim.prev
        else:
            pos, prev = m.pos, m.prev
        self.ring.append((self.steps_seen,) + frame_of(m.uids, pos, prev, self.tracked))
        self.recorded += 1

    def after_step(self):
        """The model has made one step (whoever drove it): count it, and take a frame on every every-th."""
        self.steps_seen += 1
        if self.steps_seen % self.every == 0:
            self.sample()

    def step(self, dt, resort=False):
        self.m.step(dt, resort=resort)
        self.after_step()

    def run(self, dt, steps, resort_every=0, resort_first=True):
        for s in range(steps):
            resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
            self.step(dt, resort=bool(resort))

    def read(self, capacity=None, consume=False):
        held = list(self.ring)
        count = len(held)
        give = held if capacity is None else held[count - min(count, capacity):]
        k = len(self.tracked)
        out = Frames(np.array([f[0] for f in give], np.uint64),
                     np.array([f[1] for f in give], F32).reshape(-1, k, 2),
                     np.array([f[2] for f in give], F32).reshape(-1, k, 2),
                     np.array([f[3] for f in give], np.uint32).reshape(-1, k), count, self.recorded)
        if consume:
            self.ring.clear()
        return out
