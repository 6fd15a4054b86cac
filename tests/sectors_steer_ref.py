"""The steer of include/d2pc_sectors.h (d2pc_sectors_steer_*) restated in numpy: all integers.  The reach tables are
ARGUMENTS of SectorsSteerRef (the tests hand over the library's own, d2pc_sectors_steer_reach, as the other references take
their tables); reach_tables() evaluates them directly in float64, for the test that holds the library's to it.  The
clearance is the DIRECT 2-D window of the specification: the kernel takes the separable form, so the two are checked
against each other."""
import numpy as np

NOTHING, FARTHEST = 65535, 65534
BLOCKED = 0xFFFFFFFF
NO_CANDIDATE = np.uint64(0xFFFFFFFFFFFFFFFF)
OFF = 0xFFFFFFFF


def reach_quotients(rho, theta):
    """100 rho / sin(theta) where theta < pi / 2, 100 rho where it is not, in float64 (theta > 0)."""
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(theta < np.pi / 2, 100.0 * rho / np.sin(np.minimum(theta, np.pi / 2)), 100.0 * rho)


def reach_angles(cfg, scfg):
    """-> (theta of reach_s (n_layers, Wa), theta or slab offsets of reach_l (We,), eps), float64."""
    n, layers = int(cfg.n_sectors), int(cfg.n_layers)
    wa, we = int(scfg.max_reach_sectors), int(scfg.max_reach_layers)
    lo, hi = np.float64(np.float32(cfg.u_min)), np.float64(np.float32(cfg.u_max))
    alpha = 2 * np.pi / n
    with np.errstate(all="ignore"):
        eps = (hi - lo) / np.float64(layers)
        cos_i = np.ones(layers)
        if int(cfg.layer_kind) == 1:
            cos_i = np.cos(lo + (np.arange(layers, dtype=np.float64) * (hi - lo)) / np.float64(layers) + eps / 2.0)
    k = np.arange(1, wa + 1, dtype=np.float64)
    return (k[None, :] - 0.5) * alpha * cos_i[:, None], (np.arange(1, we + 1, dtype=np.float64) - 0.5) * eps, eps


def reach_tables(cfg, scfg):
    """The reach tables in float64 numpy -> (reach_s uint16 (n_layers, Wa + 1), reach_l uint16 (We + 1), the quotients that
    were floored, as one flat float64 array)."""
    rho = np.float64(np.float32(scfg.radius))
    th_s, th_l, _ = reach_angles(cfg, scfg)
    q_s = reach_quotients(rho, th_s)
    rs = np.full((th_s.shape[0], th_s.shape[1] + 1), NOTHING, dtype=np.uint16)
    rs[:, 1:] = np.minimum(np.floor(q_s), FARTHEST).astype(np.uint16)
    rl = np.full(len(th_l) + 1, NOTHING, dtype=np.uint16)
    if int(cfg.layer_kind) == 1:
        q_l = reach_quotients(rho, th_l)
        rl[1:] = np.minimum(np.floor(q_l), FARTHEST).astype(np.uint16)
    else:
        q_l = np.zeros(0)
        rl[1:] = np.where(th_l < rho, FARTHEST, 0)
    return rs, rl, np.concatenate([q_s.reshape(-1), q_l.reshape(-1)])


def step_words(goal_sector=OFF, goal_layer=0, prev_sector=OFF, prev_layer=0):
    """The 8 uint32 words of a d2pc_sectors_steer_step."""
    return np.array([goal_sector, goal_layer, prev_sector, prev_layer, 0, 0, 0, 0], dtype=np.uint64).astype(np.uint32)


class SectorsSteerRef:
    def __init__(self, cfg, scfg, reach_s, reach_l):
        self.n, self.layers = int(cfg.n_sectors), int(cfg.n_layers)
        self.n_cells = self.n * self.layers
        self.wa, self.we = int(scfg.max_reach_sectors), int(scfg.max_reach_layers)
        self.reach_s = np.asarray(reach_s, dtype=np.int64).reshape(self.layers, self.wa + 1)
        self.reach_l = np.asarray(reach_l, dtype=np.int64).reshape(self.we + 1)
        self.free_cm, self.min_clearance_cm, self.horizon_cm = int(scfg.free_cm), int(scfg.min_clearance_cm), int(scfg.horizon_cm)
        self.w_goal, self.w_prev, self.w_near = int(scfg.w_goal), int(scfg.w_prev), int(scfg.w_near)

    def mapped(self, distance_cm):
        """d: the input with the free_cm mapping, int32 (n_layers, n_sectors)."""
        d = np.asarray(distance_cm).astype(np.int32).reshape(self.layers, self.n)
        return np.where(d >= self.free_cm, NOTHING, d)

    def clearance(self, distance_cm):
        """The direct 2-D window -> int32 (n_cells,): from the obstacles' side where they are few (a built case of one or two
        obstacles costs a millisecond), from the cells' side otherwise.  tests/test_sectors_steer_cpu.py holds the two equal."""
        few = np.count_nonzero(self.mapped(distance_cm) != NOTHING) * (2 * self.wa + 1) * (2 * self.we + 1) <= 100_000
        return self.clearance_scatter(distance_cm) if few else self.clearance_window(distance_cm)

    def clearance_scatter(self, distance_cm):
        """The same window from the obstacles' side: every obstacle (s', l') of value v lowers the cells
        ((s' - ks) mod n, l' - kl) with v <= reach_l[|kl|] and v <= reach_s[l'][|ks|]."""
        d = self.mapped(distance_cm)
        l0, s0 = np.nonzero(d != NOTHING)
        v = d[l0, s0]
        ks, kl = np.meshgrid(np.arange(-self.wa, self.wa + 1), np.arange(-self.we, self.we + 1))
        ks, kl = ks.reshape(-1), kl.reshape(-1)
        tl = l0[:, None] - kl[None, :]
        ts = np.mod(s0[:, None] - ks[None, :], self.n)
        ok = (tl >= 0) & (tl < self.layers) & (v[:, None] <= self.reach_l[np.abs(kl)][None, :]) & (v[:, None] <= self.reach_s[l0][:, np.abs(ks)])
        out = np.full(self.n_cells, NOTHING, dtype=np.int32)
        np.minimum.at(out, (tl * self.n + ts)[ok], np.broadcast_to(v[:, None], ok.shape)[ok])
        return out

    def clearance_window(self, distance_cm):
        """The direct 2-D window, from the cells' side -> int32 (n_cells,)."""
        d = self.mapped(distance_cm)
        out = np.full((self.layers, self.n), NOTHING, dtype=np.int32)
        for kl in range(-self.we, self.we + 1):
            lo, hi = max(0, -kl), min(self.layers, self.layers - kl)        # the target layers l with 0 <= l + kl < L
            if lo >= hi:
                continue
            src = d[lo + kl:hi + kl]                                        # rows l + kl
            rows = self.reach_s[lo + kl:hi + kl]                            # indexed by the SOURCE's layer
            for ks in range(-self.wa, self.wa + 1):
                v = np.roll(src, -ks, axis=1)                               # v[l, s] = d[l + kl, (s + ks) mod n]
                ok = (v <= self.reach_l[abs(kl)]) & (v <= rows[:, abs(ks)][:, None])
                out[lo:hi] = np.minimum(out[lo:hi], np.where(ok, v, NOTHING))
        return out.reshape(-1)

    def delta(self, sector, layer):
        """D(c, (sector, layer)) of every cell, int64 (n_cells,); zeros when the sector switches the term off."""
        if sector >= self.n:
            return np.zeros(self.n_cells, dtype=np.int64)
        layer = min(int(layer), self.layers - 1)
        s, l = np.meshgrid(np.arange(self.n), np.arange(self.layers))
        ds = np.abs(s - int(sector))
        return (np.minimum(ds, self.n - ds) + np.abs(l - layer)).reshape(-1)

    def steer(self, distance_cm, step, allowed=None, n_candidates=1):
        """One d2pc_sectors_steer_device.  step: the 8 words (or the first four).
        -> dict(clearance_cm uint16, cost uint32, candidates uint64 (n_candidates,), summary uint32 (4,))."""
        clr = self.clearance(distance_cm)
        free = clr >= self.min_clearance_cm
        if allowed is not None:
            free &= np.asarray(allowed).reshape(-1) != 0
        gs, gl, ps, pl = (int(w) for w in np.asarray(step).reshape(-1)[:4])
        cost = self.w_goal * self.delta(gs, gl) + self.w_prev * self.delta(ps, pl) + self.w_near * (
            self.horizon_cm - np.minimum(clr, self.horizon_cm))
        assert cost.max() < BLOCKED
        cost = np.where(free, cost, BLOCKED)
        keys = np.sort((cost[free].astype(np.uint64) << np.uint64(32)) | np.flatnonzero(free).astype(np.uint64))
        cand = np.full(n_candidates, NO_CANDIDATE, dtype=np.uint64)
        cand[:min(n_candidates, len(keys))] = keys[:n_candidates]
        summary = np.array([free.sum(), self.mapped(distance_cm).min(), 0, 0], dtype=np.uint32)
        return dict(clearance_cm=clr.astype(np.uint16), cost=cost.astype(np.uint32), candidates=cand, summary=summary)
