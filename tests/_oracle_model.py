"""A CPU model of one gpe context, built on the C oracle (oracle/oracle.py).  TEST INFRASTRUCTURE ONLY.

OracleModel holds what a context holds, in storage order: pos, prev, radius, the uids and next_uid (uids on), and the
constants a step depends on (world, gravity, mouse, the grid radius and the max radius).  Each public operation of
include/gpe.h is applied as the header and the API's host side (csrc/gpe_api.hip, gpe_queries.hip, gpe_edits.hip,
gpe_observe.hip) define it; the steps themselves run through oracle.Sim.
Whenever a constant or the arrays change on the host side, the next step builds a new Sim from the current arrays
(with prev=), so a Sim never sees stale constants.  The step keeps no hidden state between calls (home cells and
particle ids are rebuilt by every re-sort), which tests/test_oracle_model_cpu.py checks against one long-lived Sim.
"""
import collections

import numpy as np

from tests import _clusters_model, _contacts_model, _spawn_model

F32 = np.float32
VEL_ADD, VEL_SET, VEL_SCALE = 0, 1, 2    # GPE_VEL_*
# what the read-only calls deliver (the engine's QueryResult / ContactResult / ClusterResult, uid fields None while
# uids are off)
Rows = collections.namedtuple("Rows", "index uid pos prev radius")
Contacts = collections.namedtuple("Contacts", "count degree a b uid_a uid_b overlap")
Clusters = collections.namedtuple("Clusters", "label size label_uid count largest_size largest_label")
CELL_SIZE_MULTIPLIER = F32(2.2)          # gpe_config_default, grid.rs:20


def max_abs_radius(radius):
    """gpe_set_particles / removal: the radius of largest magnitude, the LAST of several, sign kept (max_by)."""
    r = np.ascontiguousarray(radius, F32)
    best = r[0]
    for v in r:
        if not (abs(v) < abs(best)):
            best = v
    return F32(best)


def circle_mask(pos, x, y, radius):
    """gpe_remove_particles_in_circle: (p.x-x)^2 + (p.y-y)^2 <= radius^2, binary32, left to right, no FMA."""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    dx = p[:, 0] - F32(x)
    dy = p[:, 1] - F32(y)
    return (dx * dx + dy * dy) <= F32(radius) * F32(radius)


def box_mask(pos, x0, y0, x1, y1):
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    return (F32(x0) <= p[:, 0]) & (p[:, 0] <= F32(x1)) & (F32(y0) <= p[:, 1]) & (p[:, 1] <= F32(y1))


def pick_oracle(pos, rad, x, y):
    """argmin over (bits(d2), index) of the particles whose own disc contains (x, y), binary32 without FMA"""
    p = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    r = np.ascontiguousarray(rad, F32)
    dx = p[:, 0] - F32(x)
    dy = p[:, 1] - F32(y)
    d2 = dx * dx + dy * dy
    inside = np.nonzero(d2 <= r * r)[0]
    if inside.size == 0:
        return None
    keys = (d2[inside].view(np.uint32).astype(np.uint64) << np.uint64(32)) | inside.astype(np.uint64)
    return int(inside[np.argmin(keys)])


def kicked_prev(op, pos, prev, mask, a):
    """The numpy float32 formula of include/gpe.h on the masked set, one rounding per operation."""
    out = prev.copy()
    for c in (0, 1):
        p, q, ac = pos[mask, c], prev[mask, c], F32(a[c])
        if op == VEL_ADD:
            out[mask, c] = q - ac
        elif op == VEL_SET:
            out[mask, c] = p - ac
        else:
            v = p - q
            v = v * ac
            out[mask, c] = p - v
    return out


class OracleModel:
    def __init__(self, oracle, pos, radius, world=(3048.0, 1048.0), gravity=(0.0, 0.0), prev=None):
        self.o = oracle
        self.pos = np.array(pos, F32).reshape(-1, 2)
        self.prev = self.pos.copy() if prev is None else np.array(prev, F32).reshape(-1, 2)
        self.radius = np.array(radius, F32).reshape(-1)
        assert self.pos.shape[0] == self.radius.shape[0] > 0
        self.world = (F32(world[0]), F32(world[1]))
        self.gravity = (F32(gravity[0]), F32(gravity[1]))
        self.mouse = (False, (F32(0.0), F32(0.0)))
        self.max_radius = max_abs_radius(self.radius)          # gpe_set_particles
        self.grid_max_radius = self.max_radius
        self.uids = None                                       # None: uids off
        self.next_uid = None
        self._sim = None
        self._searched = None

    # ---- the state as a context reports it ----------------------------------------------------------------------
    def __len__(self):
        return self.pos.shape[0]

    @property
    def cell_size(self):
        return F32(self.grid_max_radius * CELL_SIZE_MULTIPLIER)   # refresh_cell_size

    def arrays(self):
        self._pull()
        return self.pos, self.prev, self.radius

    # ---- the Sim behind the steps -------------------------------------------------------------------------------
    def _params(self):
        p = self.o.default_params(float(self.world[0]), float(self.world[1]), 1.0)
        p.cell_size = float(self.cell_size)
        p.gravity_x, p.gravity_y = float(self.gravity[0]), float(self.gravity[1])
        p.mouse_pressed = 1 if self.mouse[0] else 0
        p.mouse_x, p.mouse_y = float(self.mouse[1][0]), float(self.mouse[1][1])
        return p

    def sim(self):
        if self._sim is None:
            self._sim = self.o.Sim(self.pos, self.radius, self._params(), prev=self.prev)
        return self._sim

    def _pull(self):
        """Take the arrays back from the Sim and drop it (a host-side change follows)."""
        if self._sim is not None:
            self.pos, self.prev, self.radius = self._sim.pos, self._sim.prev, self._sim.radius
            self._sim.close()
            self._sim = None

    # ---- steps, module calls, re-sort ---------------------------------------------------------------------------
    def step(self, dt, resort=False):
        if resort and self.uids is not None:
            self.morton_resort()                       # (what Sim.step's re-sort does, with the uids following)
            resort = False
        self.sim().step(dt, resort=resort)

    def run(self, dt, steps, resort_every=0, resort_first=True):
        """gpe_run: the re-sort before step 0 (resort_first) and before every step s > 0 with s % resort_every == 0."""
        for s in range(steps):
            resort = (s == 0 and resort_first) or (resort_every and s > 0 and s % resort_every == 0)
            self.step(dt, resort=bool(resort))

    def module_calls(self, dt):
        """Grid::update, CollisionSystem::solve_collisions, ParticleSystem::update_positions, one call each."""
        sim = self.sim()
        sim.grid_build(); sim.grid_sort()
        sim.build_collision_cells(); sim.solve_colors()
        sim.integrate(dt)

    def morton_resort(self):
        sim = self.sim()
        sim.morton_resort()
        if self.uids is not None:                  # the uids travel with their particles: new[i] = old[ids[i]]
            self.uids = self.uids[sim.particle_ids]

    # ---- particles ----------------------------------------------------------------------------------------------
    def add(self, pos, radius):
        """gpe_add_particles: appended with prev = pos; max_radius = fmaxf(max_radius, r) over the new radii in
        order, and the grid radius follows it (Grid::refresh_grid)."""
        self._pull()
        p = np.array(pos, F32).reshape(-1, 2)
        r = np.array(radius, F32).reshape(-1)
        if p.shape[0] == 0:
            return
        self.pos = np.concatenate([self.pos, p])
        self.prev = np.concatenate([self.prev, p])
        self.radius = np.concatenate([self.radius, r])
        m = self.max_radius
        for v in r:
            m = F32(np.fmax(m, v))
        self.max_radius = m
        self.grid_max_radius = m
        if self.uids is not None:
            k = p.shape[0]
            self.uids = np.concatenate([self.uids, np.arange(self.next_uid, self.next_uid + k, dtype=np.uint64)
                                        .astype(np.uint32)])
            self.next_uid += k

    def _remove(self, gone):
        self._pull()
        gone = np.asarray(gone, bool)
        k = int(gone.sum())
        if k == 0:
            return 0                                   # untouched, grid radius included
        if k == len(self):
            raise ValueError("the context refuses to remove every particle")
        keep = ~gone
        self.pos, self.prev, self.radius = self.pos[keep], self.prev[keep], self.radius[keep]
        if self.uids is not None:
            self.uids = self.uids[keep]
        self.max_radius = max_abs_radius(self.radius)
        self.grid_max_radius = self.max_radius
        return k

    def remove_mask(self, mask):
        return self._remove(np.asarray(mask) != 0)

    def remove_circle(self, x, y, radius):
        self._pull()
        return self._remove(circle_mask(self.pos, x, y, radius))

    def remove_uids(self, uids):
        assert self.uids is not None
        return self._remove(np.isin(self.uids, np.asarray(uids, np.uint32)))

    def add_free(self, cpos, crad, separate=False, inside_world=False, dry_run=False):
        """gpe_add_particles_free -> (verdict u8[k], added): the verdicts of tests/_spawn_model.spawn against the
        particles as they are, then -- unless dry_run -- add() of the ADDED rows.  A dry run and added == 0 change
        nothing, a grid override included (add() of no rows returns before it touches anything)."""
        self._pull()
        verdict, p_new, r_new = _spawn_model.spawn(self.pos, self.radius, cpos, crad, self.world, separate=separate,
                                                   inside_world=inside_world)
        if not dry_run:
            self.add(p_new, r_new)
        return verdict, int(r_new.shape[0])

    def edit(self, keys, by, pos=None, prev=None, radius=None):
        """gpe_edit_particles -> edited.  by: "index" or "uid"; absent uids are skipped; row i of every array given goes
        to the particle key i names; pos without prev puts the particle at rest (prev = pos).  radius given: max_radius
        is recomputed over all particles and the grid radius follows it; radius None: both untouched, an override
        included.  Uids and order are kept."""
        assert by in ("index", "uid") and not (pos is None and prev is None and radius is None)
        keys = np.asarray(keys, np.uint32).reshape(-1)
        if by == "uid":
            assert self.uids is not None
            order = np.argsort(self.uids, kind="stable")
            at = np.searchsorted(self.uids[order], keys)
            at[at == len(order)] = 0
            found = self.uids[order[at]] == keys
            rows, who = np.nonzero(found)[0], order[at[found]]
        else:
            assert (keys < len(self)).all()
            rows, who = np.arange(len(keys)), keys.astype(np.int64)
        assert len(np.unique(who)) == len(who), "two keys name one particle: the context refuses that"
        if len(keys) == 0:
            return 0
        self._pull()
        if pos is not None:
            p = np.asarray(pos, F32).reshape(-1, 2)[rows]
            self.pos = self.pos.copy(); self.pos[who] = p
            if prev is None:
                self.prev = self.prev.copy(); self.prev[who] = p
        if prev is not None:
            self.prev = self.prev.copy(); self.prev[who] = np.asarray(prev, F32).reshape(-1, 2)[rows]
        if radius is not None:
            self.radius = self.radius.copy(); self.radius[who] = np.asarray(radius, F32).reshape(-1)[rows]
            self.max_radius = max_abs_radius(self.radius)
            self.grid_max_radius = self.max_radius
        return int(len(who))

    def kick(self, mask, op, ax, ay):
        """gpe_kick_circle / gpe_kick_box on the particles of `mask` (circle_mask / box_mask of the current positions):
        prev only, by the float32 formulas of GPE_VEL_ADD / SET / SCALE.  Returns the number kicked."""
        self._pull()
        mask = np.asarray(mask, bool)
        self.prev = kicked_prev(op, self.pos, self.prev, mask, (ax, ay))
        return int(mask.sum())

    # ---- read-only queries: the rows a context returns ----------------------------------------------------------
    def rows(self, index):
        self._pull()
        index = np.asarray(index, np.int64).reshape(-1)
        return Rows(index.astype(np.uint32), None if self.uids is None else self.uids[index], self.pos[index],
                    self.prev[index], self.radius[index])

    def query_circle(self, x, y, radius):
        self._pull()
        return self.rows(np.nonzero(circle_mask(self.pos, x, y, radius))[0])

    def query_box(self, x0, y0, x1, y1):
        self._pull()
        return self.rows(np.nonzero(box_mask(self.pos, x0, y0, x1, y1))[0])

    def pick(self, x, y):
        """gpe_pick: the rows of the one particle picked, or None."""
        self._pull()
        i = pick_oracle(self.pos, np.abs(self.radius), x, y)
        return None if i is None else self.rows([i])

    def _contacts(self):
        """The brute-force search, kept for as long as pos and radius hold the same bits (a contact and a cluster
        query on one state search once)."""
        self._pull()
        key = (self.pos.tobytes(), self.radius.tobytes())
        if self._searched is None or self._searched[0] != key:
            found = _contacts_model.contacts(self.pos, self.radius)
            label = _clusters_model.labels_from_pairs(len(self), found[2], found[3])
            self._searched = (key, found, label)
        return self._searched[1]

    def contacts(self):
        """gpe_query_contacts: every pair (a caller cuts the per-pair arrays to its capacity)."""
        count, degree, a, b, overlap = self._contacts()
        ua = ub = None
        if self.uids is not None:
            ua, ub = self.uids[a], self.uids[b]
        return Contacts(count, degree, a, b, ua, ub, overlap)

    def clusters(self):
        self._contacts()
        label = self._searched[2]
        size, count, largest_size, largest_label = _clusters_model.summary(label)
        return Clusters(label, size, None if self.uids is None else self.uids[label], count, largest_size,
                        largest_label)

    def cluster_of(self, index=None, uid=None, label=None):
        """gpe_query_cluster_of: the members of the cluster of particle `index`, or of the particle with `uid` (no rows
        for an absent uid), ascending.  label: the labels of clusters(), when the caller has them already."""
        assert (index is None) != (uid is None)
        self._pull()
        if uid is not None:
            at = np.nonzero(self.uids == np.uint32(uid))[0]
            if at.size == 0:
                return self.rows([])
            index = int(at[0])
        if label is None:
            label = self.clusters().label
        return self.rows(np.nonzero(label == label[index])[0])

    # ---- constants ----------------------------------------------------------------------------------------------
    def set_world(self, w, h):
        self._pull()
        self.world = (F32(w), F32(h))

    def set_gravity(self, gx, gy):
        self._pull()
        self.gravity = (F32(gx), F32(gy))

    def set_mouse(self, pressed, x, y):
        self._pull()
        self.mouse = (bool(pressed), (F32(x), F32(y)))

    def grid_set_max_radius(self, r):
        """Lasts until the next set / add / remove (or the next call)."""
        self._pull()
        self.grid_max_radius = F32(r)

    def set_mode(self, mode):
        pass                                           # a pipeline choice: same bits

    # ---- uids ---------------------------------------------------------------------------------------------------
    def enable_uids(self, on=True):
        if not on:
            self.uids = self.next_uid = None
        elif self.uids is None:
            self.uids = np.arange(len(self), dtype=np.uint32)
            self.next_uid = len(self)

    def set_uids(self, uids):
        u = np.array(uids, np.uint32).reshape(-1)
        assert u.shape[0] == len(self) and len(np.unique(u)) == len(u)
        self.uids = u
        self.next_uid = int(u.max()) + 1

    def set_next_uid(self, next_uid):
        assert self.uids is not None and int(self.uids.max()) < next_uid <= 1 << 32
        self.next_uid = int(next_uid)

    # ---- writes through gpe_device_ptr --------------------------------------------------------------------------
    def stop_all(self):
        """prev = pos for every particle."""
        self._pull()
        self.prev = self.pos.copy()

    def teleport(self, who, where):
        """pos and prev of the particles `who` set to `where` (inside the current box)."""
        self._pull()
        self.pos = self.pos.copy(); self.prev = self.prev.copy()
        self.pos[who] = where
        self.prev[who] = where

    def close(self):
        if self._sim is not None:
            self._sim.close()
            self._sim = None
