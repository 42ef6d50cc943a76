"""A CPU model of one gpe context, built on the C oracle (oracle/oracle.py).  TEST INFRASTRUCTURE ONLY.

OracleModel holds what a context holds, in storage order: pos, prev, radius, the uids and next_uid (uids on), and the
constants a step depends on (world, gravity, mouse, the grid radius and the max radius).  Each public operation of
include/gpe.h is applied as the header and csrc/gpe_api.hip define it; the steps themselves run through oracle.Sim.
Whenever a constant or the arrays change on the host side, the next step builds a new Sim from the current arrays
(with prev=), so a Sim never sees stale constants.  The step keeps no hidden state between calls (home cells and
particle ids are rebuilt by every re-sort), which tests/test_oracle_model_cpu.py checks against one long-lived Sim.
"""
import numpy as np

F32 = np.float32
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
