"""The numpy float32 restatement of gpe_add_particles_free (include/gpe.h): brute force, in the exact operation order of
the header.  Contact is the predicate of gpe_query_contacts with the candidate first -- dx = xc - xp, dy = yc - yp,
q = dx*dx + dy*dy, rs = rc + rp, contact when q < rs*rs -- one binary32 rounding per operation, no FMA (numpy rounds every
array operation once).  The world test is a = |r|; x >= a and x <= W - a and y >= a and y <= H - a.  The separation is
the sequential greedy loop over ascending input index.  Row blocks keep the memory bounded."""
import numpy as np

F32 = np.float32
ADDED, BLOCKED_BY_PARTICLE, BLOCKED_BY_CANDIDATE, OUTSIDE_WORLD = 0, 1, 2, 3


def touches(cpos, crad, pos, rad):
    """hit[i, j]: candidate i is in contact with particle j (K x N, bool)"""
    with np.errstate(all="ignore"):                                   # (in place: the same roundings, fewer arrays)
        q = np.subtract.outer(cpos[:, 0], pos[:, 0])
        np.multiply(q, q, out=q)
        dy = np.subtract.outer(cpos[:, 1], pos[:, 1])
        np.multiply(dy, dy, out=dy)
        np.add(q, dy, out=q)
        rs = np.add.outer(crad, rad)
        np.multiply(rs, rs, out=rs)
        return q < rs


def outside_world(cpos, crad, world):
    with np.errstate(all="ignore"):
        a = np.abs(crad)
        wx, wy = F32(world[0]) - a, F32(world[1]) - a
        x, y = cpos[:, 0], cpos[:, 1]
        return ~((x >= a) & (x <= wx) & (y >= a) & (y <= wy))


def spawn(pos, rad, cpos, crad, world, separate=False, inside_world=False, block=128):
    """-> (verdict u8[k], appended pos f32[added, 2], appended radius f32[added]): the verdict of every candidate and the
    rows gpe_add_particles would be given, in input order"""
    pos = np.ascontiguousarray(pos, F32).reshape(-1, 2)
    rad = np.ascontiguousarray(rad, F32).reshape(-1)
    cpos = np.ascontiguousarray(cpos, F32).reshape(-1, 2)
    crad = np.ascontiguousarray(crad, F32).reshape(-1)
    k = crad.shape[0]
    verdict = np.zeros(k, np.uint8)
    for lo in range(0, k, block):                                     # rule 2
        hi = min(lo + block, k)
        verdict[lo:hi][touches(cpos[lo:hi], crad[lo:hi], pos, rad).any(axis=1)] = BLOCKED_BY_PARTICLE
    if inside_world:                                                  # rule 1 wins over rule 2
        verdict[outside_world(cpos, crad, world)] = OUTSIDE_WORLD
    if separate:                                                      # rule 3: the sequential greedy loop
        taken = np.zeros(k, bool)                                     # ADDED so far
        for i in range(k):
            if verdict[i] != ADDED:
                continue
            lower = np.nonzero(taken[:i])[0]
            if lower.size and touches(cpos[i:i + 1], crad[i:i + 1], cpos[lower], crad[lower]).any():
                verdict[i] = BLOCKED_BY_CANDIDATE
            else:
                taken[i] = True
    keep = verdict == ADDED
    return verdict, cpos[keep].copy(), crad[keep].copy()


def max_radius_after(max_radius, appended_radius):
    """gpe_max_radius after the append: fmaxf over the appended radii, in input order"""
    m = F32(max_radius)
    for r in np.asarray(appended_radius, F32):
        m = np.fmax(m, r)
    return F32(m)


def reference_spray(rng, centre, k):
    """k candidates as the reference's add_particles sprays them round a point (particle_system.rs:163-220): a random
    angle, a distance of 10 .. 50 + 1.5 (i mod 100), a radius of 1, 2 or 3"""
    angle = rng.uniform(0.0, 2.0 * np.pi, k)
    dist = rng.uniform(10.0, 50.0 + 1.5 * (np.arange(k) % 100))
    cpos = np.stack([centre[0] + dist * np.cos(angle), centre[1] + dist * np.sin(angle)], axis=1).astype(F32)
    crad = rng.integers(1, 4, k).astype(F32)
    return cpos, crad
