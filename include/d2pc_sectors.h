/*
 * d2pc_sectors.h -- C ABI of the OBSTACLE SECTORS: a polar min-range grid made on the device from any cloud this
 * project produces.  The companion library libd2pc_sectors.so exports it; it links the HIP runtime only and needs
 * nothing of libd2pc.so or of a d2pc_ctx (this header includes d2pc.h for d2pc_status alone).
 *
 * A cloud of an omnidirectional rig exists so that an avoidance stack can ask "how far is the nearest obstacle in each
 * direction": the 72-sector OBSTACLE_DISTANCE record of MAVLink, the polar histogram a local planner builds first.
 * This call answers it behind the producer, on the producer's stream, and leaves n_sectors x n_layers cells in device
 * memory -- 144 bytes for the default grid instead of the 50-70 MB of the cloud.
 *
 * Plain C: pointers and sizes only.  Every function returns a d2pc_status and never throws or aborts.  No CPU path:
 * without a usable gfx950 device d2pc_sectors_create fails with D2PC_ERR_NO_DEVICE.  A session is not thread-safe.
 *
 * ---------------------------------------------------------------------------------------------------- SPECIFICATION
 * Exact, so that float32 arithmetic with ONE rounding per operation (no fused multiply-add) reproduces every bit;
 * fl() below is that rounding.  tests/sectors_ref.py restates it in numpy.
 *
 * Per point.  The record's first three floats are x, y, z.  axes[3] picks forward, left and up from them: each pick is
 * +-1, +-2 or +-3 (x, y, z; a negative pick negates, which is exact) and the magnitudes are distinct:
 *     f = pick(axes[0]),  l = pick(axes[1]),  u = pick(axes[2])
 * The optical frame of a camera (x right, y down, z forward) is {+3, -1, -2}; a body frame x forward, y left, z up is
 * {+1, +2, +3}.  Negating the pick of `l` makes the sectors run clockwise seen from above (MAVLink's numbering).
 *
 * Gate.  A point takes part if and only if
 *     x, y and z are finite
 *     r2 = fl(fl(f*f) + fl(l*l)) > 0
 *     rmin2 <= r2 <= rmax2,  rmin2 = fl(r_min*r_min), rmax2 = fl(r_max*r_max) formed once on the host (r_max = +inf
 *                            is allowed; so is r2 = +inf then)
 *     u_min <= u < u_max     (-inf / +inf: no gate; both finite and u_min < u_max when n_layers > 1)
 *
 * Layer.  0 when n_layers = 1, otherwise min(n_layers - 1, (int)floorf(fl(fl(u - u_min) * inv_h))) with
 *     inv_h = (float)(n_layers / ((double)u_max - (double)u_min)), formed on the host (d2pc_sectors_geometry returns it)
 *
 * Sector.  n = n_sectors is even.  azimuth0 (radians, double) is the direction of the boundary between the last sector
 * and sector 0, measured from f towards l.  The boundary table holds n/2 directions, evaluated in double and rounded
 * once:  c_j = (float)cos(azimuth0 + 2 pi j / n),  s_j = (float)sin(azimuth0 + 2 pi j / n),  j = 0 .. n/2 - 1
 * (d2pc_sectors_table returns it).  With
 *     cross_j(f, l) = fl(fl(c_j*l) - fl(s_j*f))          dot_0 = fl(fl(c_0*f) + fl(s_0*l))
 *     h  = cross_0 < 0  or  (cross_0 == 0 and dot_0 < 0)       the far half: if h, negate f and l
 *     k' = the number of j in 1 .. n/2 - 1 with cross_j(f, l) >= 0
 * the sector is k' + h * n/2.  This COUNT is the definition: it is total and needs no atan2, whatever rounding does to
 * a point next to a boundary; away from a boundary it is the sector float64 atan2 binning gives.
 *
 * Cell.  cell = layer * n_sectors + sector.  Its key is the minimum, as an unsigned 64-bit number, over the cell's
 * points of (bits(r2) << 32) | position, where position = cloud * points_frame_stride_points + record is the point's
 * place in `points`.  Non-negative floats order as their bit patterns, so the key holds the smallest r2 and, among
 * equal r2, the smallest position: the result does not depend on the order in which the device visits the points.
 * The empty key is all ones.  All clouds of a call reduce into ONE grid: they are one instant of one vehicle.
 *
 * Outputs, n_cells entries each, all nullable but one:
 *     range        float32  sqrtf(smallest r2), correctly rounded; +inf when count < min_count
 *     count        uint32   the cell's points
 *     nearest      uint32   the key's low word (the position of the closest point); 0xFFFFFFFF for an empty cell;
 *                           NOT masked by min_count
 *     distance_cm  uint16   no_obstacle_cm when count < min_count, otherwise fl(range * 100.0f) truncated towards zero
 *                           and clamped to 65534 (OBSTACLE_DISTANCE's form; MAVLink asks for max_distance + 1 where
 *                           nothing is seen; marking sectors no camera covers as 65535 is the caller's)
 *
 * ------------------------------------------------------------------------------- ELEVATION LAYERS (layer_kind = 1)
 * The layers above are height slabs and the range is the horizontal one: what OBSTACLE_DISTANCE asks for.  A local
 * planner's polar histogram is azimuth x ELEVATION ANGLE (typically 60 x 30 cells of 6 degrees) and holds the Euclidean
 * distance of the nearest point in each direction.  With layer_kind = D2PC_SECTORS_LAYERS_ELEVATION the picks, the
 * sector, the cell's place, the empty key and the four outputs are as above; what changes is this.  tests/
 * sectors_elev_ref.py restates it in numpy.
 *
 * Boundaries.  u_min and u_max are the elevation band in radians, measured from the horizontal plane towards u, both
 * within [-1.5707964f, +1.5707964f] (the float nearest pi/2) and u_min < u_max; there is no height gate.  With n =
 * n_layers (1 .. D2PC_SECTORS_MAX_ELEVATION_LAYERS) the n + 1 boundary elevations are, in double,
 *     e_i = (double)u_min + ((double)i * ((double)u_max - (double)u_min)) / (double)n,   i = 0 .. n
 * and the elevation table holds  ce_i = (float)cos(e_i),  se_i = (float)sin(e_i), evaluated in double and rounded once
 * on the host (d2pc_sectors_elevation_table returns it).
 *
 * Per point.  r2 as above, then
 *     h   = sqrtf(r2), correctly rounded            d2 = fl(r2 + fl(u*u))
 *     t_i = fl(fl(ce_i*u) - fl(se_i*h))             (the sine of the point's elevation above boundary i, times its range)
 *
 * Gate.  x, y and z are finite;  r2 > 0 (a point on the vertical axis has no azimuth);  rmin2 <= d2 <= rmax2 (the range
 * gate is on the EUCLIDEAN range; r_max = +inf is allowed, and d2 = +inf with it);  t_0 >= 0  and  not (t_n >= 0) --
 * exactly so: a NaN t (0 * inf: h = +inf against a boundary at elevation 0) takes no part in any comparison.
 *
 * Layer.  The number of i in 1 .. n - 1 with t_i >= 0.  Like the sector this COUNT is the definition: it is total and
 * needs no atan2; away from a boundary it is the layer float64 atan2(u, hypot(f, l)) binning gives.  cell = layer *
 * n_sectors + sector, the lowest elevation first.
 *
 * Key.  (bits(d2) << 32) | position: the smallest Euclidean d2 and, among equal d2, the smallest position.
 * range = sqrtf(smallest d2); count, nearest and distance_cm are formed from the key and the range exactly as above.
 *
 * ------------------------------------------------------------------------------------- MEMORY (d2pc_sectors_memory_*)
 * One forward camera fills a few cells of a 360-degree grid; a wall the vehicle yawed away from is gone one frame later.
 * A memory session keeps ONE point per cell in a fixed (world) frame between calls, as a local planner's histogram
 * memory does.  d2pc_sectors_memory_update_device takes what d2pc_sectors_process_device wrote for a cloud (count,
 * nearest), the cloud and a pose, re-bins the remembered points under the new pose, ages them and merges them with the
 * cells seen now.  The gate, layer, sector and cell of a remembered point are the definitions above, with the same
 * tables and the same comparisons: it lands in exactly the cell the grid itself would put it in.
 * tests/sectors_memory_ref.py restates this in numpy.
 *
 * A record is 16 bytes: the world x, y, z as float32 and the age as uint32, in the caller's ticks.  The empty record is
 * the words 0, 0, 0, 0xFFFFFFFF.  The step (d2pc_sectors_memory_step, in DEVICE memory) holds R (row-major), t and dt:
 * world = R p + t for a point p in the frame of `points`; dt is the ticks since the previous update.
 *
 * Carry.  For every non-empty remembered record i (world w, age a):
 *     1. a' = min(a + dt, 0xFFFFFFFE), formed without wrap; the record is dropped if a' > max_age
 *     2. d = (fl(w.x - t.x), fl(w.y - t.y), fl(w.z - t.z))
 *     3. p.x = fl(fl(fl(R[0]*d.x) + fl(R[3]*d.y)) + fl(R[6]*d.z)),  p.y likewise with R[1], R[4], R[7],  p.z with R[2],
 *        R[5], R[8]: the transpose of R
 *     4. p goes through the gate, layer and sector of the session's layer kind exactly as a record x, y, z above does
 *        (the picks, the tables, every comparison); it is dropped if it takes no part
 *     5. it is dropped if `covered` is given and covered[cell] != 0
 *     6. otherwise the cell's carry key is the minimum, as an unsigned 64-bit number, of (bits(k) << 32) | i with k = r2
 *        for height layers and k = d2 for elevation layers
 *
 * Merge, per cell c.  The cell is FRESH when count[c] >= min_count and nearest[c] is below the call's position bound
 * (n_clouds - 1) * points_frame_stride_points + cloud_points (cloud_points for one cloud).  A `nearest` at or above the
 * bound counts as not seen; nothing is read there.
 *     fresh              q = the record at position nearest[c].  The new record is
 *                        (fl(fl(fl(fl(R[0]*q.x) + fl(R[1]*q.y)) + fl(R[2]*q.z)) + t.x), likewise with R[3..5] and t.y,
 *                        with R[6..8] and t.z, age 0) and range = sqrtf(k(q)) with k formed from the picks of q as
 *                        above: the bits d2pc_sectors_process_device wrote to range[c]
 *     not fresh, a key   the new record is record i (the key's low word) unchanged with the age a';
 *                        range = sqrtf(the key's high word).  min_count does not apply to a remembered cell
 *     otherwise          the empty record; range = +inf
 * distance_cm is formed from range as above, no_obstacle_cm where the record is empty; age[c] is the record's age word.
 * The new records replace the old as one step: no carry reads a record this call wrote.
 *
 * --------------------------------------------------------------------------------------- STEER (d2pc_sectors_steer_*)
 * What a consumer of the grid does first: widen every obstacle by the vehicle's radius (VFH+'s enlargement), mask the
 * directions that are no longer free and rank the free ones against a goal direction, the previous heading and the
 * clearance.  d2pc_sectors_steer_device does it in one launch from a grid's distance_cm, as d2pc_sectors_process_device
 * or d2pc_sectors_memory_update_device wrote it, for either layer kind.  All integers: nothing is rounded on the device.
 * tests/sectors_steer_ref.py restates it in numpy.
 *
 * Grid.  n = n_sectors, L = n_layers, cell (s, l) = l * n + s.  Sectors wrap around; layers do not (no over-the-pole
 * neighbour).
 *
 * Input.  d[c] = distance_cm[c]; a value >= free_cm is read as 65535, nothing there (a no_obstacle_cm that is not 65535).
 *
 * Reach tables, made once on the host in double (d2pc_sectors_steer_reach returns them).  rho = (double)radius (the
 * vehicle's radius plus margin), alpha = 2 pi / n, Wa = max_reach_sectors, We = max_reach_layers, and
 *     reach(theta) = min(65534, floor(100 rho / sin(theta)))  for 0 < theta < pi/2,
 *                    min(65534, floor(100 rho))               for theta >= pi/2    (65534 for a theta that is not > 0)
 *     reach_s[i][0] = reach_l[0] = 65535                      (a cell always sees itself)
 *     reach_s[i][k] = reach((k - 1/2) alpha cos_i), k = 1 .. Wa, indexed by the layer i of the OBSTACLE's cell:
 *                     cos_i = 1 for height layers; cos(e_i + eps/2) for elevation layers, with e_i as the elevation
 *                     table forms it and eps = ((double)u_max - (double)u_min) / L (an obstacle near the pole spans
 *                     more sectors)
 *     reach_l[k],  k = 1 .. We:  elevation layers reach((k - 1/2) eps);  height layers 65534 if (k - 1/2) eps < rho,
 *                     otherwise 0 (eps is the slab's height then)
 *
 * Clearance.  clearance_cm[(s, l)] = the minimum of d[((s + ks) mod n, l + kl)] over |ks| <= Wa, |kl| <= We,
 * 0 <= l + kl < L, of the values v with v <= reach_l[|kl|] and v <= reach_s[l + kl][|ks|]; 65535 if none qualifies.
 * This 2-D window is the definition.  Because reach_s is indexed by the source's layer it equals an azimuth pass per
 * layer followed by a layer pass over the first pass's minima, which is what the kernel does.
 *
 * Free.  A cell is free when clearance_cm >= min_clearance_cm and (`allowed` is NULL or allowed[c] != 0).
 *
 * Step (d2pc_sectors_steer_step, 32 bytes in DEVICE memory).  A sector >= n (0xFFFFFFFF by convention) switches that term
 * off; a layer >= L is clamped to L - 1.  The kernel refuses nothing.
 *
 * Cost of a free cell, in uint32 (it cannot wrap: the weights are <= 4095):
 *     cost = w_goal * D(c, goal) + w_prev * D(c, prev) + w_near * (horizon_cm - min(clearance_cm[c], horizon_cm))
 *     D((s, l), (s', l')) = min(|s - s'|, n - |s - s'|) + |l - l'|
 * A cell that is not free has the cost 0xFFFFFFFF.
 *
 * Outputs, all nullable but one:
 *     clearance_cm  uint16 x n_cells
 *     cost          uint32 x n_cells
 *     candidates    n_candidates records {cell, cost}: as a little-endian uint64 a record is the key (cost << 32) | cell.
 *                   The list holds the smallest keys among the free cells, ascending: ties in cost go to the smaller
 *                   cell, whatever order the device visits the cells in.  Slots beyond the free cells hold all ones
 *     summary       uint32 x 4: the number of free cells, the smallest d after the free_cm mapping (65535 if none), 0, 0
 *
 * ------------------------------------------------------------------------------------- GROUND (d2pc_sectors_ground_*)
 * What a landing planner asks: "is the ground under me flat enough to land on, and where?".  A Cartesian grid of n_a x n_b
 * cells in a gravity-levelled world frame; each cell holds the number of its points, the sum of their heights and the sum
 * of the squares, in integers.  A cell is flat when it has enough points and a small spread; a site is a cell whose whole
 * neighbourhood is flat and level with it.  d2pc_sectors_ground_process_device makes it from any cloud and a pose, in at
 * most three launches.  Every accumulated value is an integer: the result is the same bytes whatever order the device
 * visits the points in.  tests/sectors_ground_ref.py restates it in numpy.
 *
 * Step (d2pc_sectors_ground_step, 80 bytes in DEVICE memory, 4-byte aligned):  float R[9], row-major: world = R p + t, as
 * the memory's step has it;  float t[3];  float origin[3] = a0, b0, h0: a0, b0 are the grid's corner, h0 is the
 * reference height (the vehicle's altitude, or the last ground estimate);  uint32 goal_i, goal_j;  uint32 reserved[3].
 * The kernel refuses nothing of a step.
 *
 * Per record.
 *     1. The record's first three floats are x, y, z.  It takes part only if all three are finite.
 *     2. w.x = fl(fl(fl(fl(R[0]*x) + fl(R[1]*y)) + fl(R[2]*z)) + t.x),  w.y likewise with R[3..5] and t.y,  w.z likewise
 *        with R[6..8] and t.z: the memory's "fresh" formula, word for word.
 *     3. axes[3] picks a, b, h from w as the sectors' picks do: +-1, +-2, +-3 of distinct magnitudes.  ENU with z up is
 *        {1, 2, 3}; NED is {1, 2, -3}.
 *     4. va = fl(fl(a - a0) * inv_c),  vb = fl(fl(b - b0) * inv_c),  inv_c = (float)(1.0 / (double)cell_size) formed on
 *        the host.
 *     5. v = fl(fl(h - h0) * inv_q),  inv_q = (float)(1.0 / (double)quantum).
 *     6. Gate, exactly so (a NaN passes no comparison):  va >= 0.0f and va < (float)n_a;  vb >= 0.0f and vb < (float)n_b;
 *        v >= -32767.0f and v <= 32767.0f.  All comparisons are in float, before any conversion.
 *     7. ia = (int)floorf(va),  ib = (int)floorf(vb),  cell = ib * n_a + ia.
 *     8. k = (int)rintf(v), round half to even, so |k| <= 32767.
 *
 * Cell.  Over the points that take part, from all clouds of the call:  count (uint32);  sum = the sum of k (int64);
 * sum2 = the sum of k*k (uint64; below 2^62, because a call holds fewer than 2^32 positions).  Sums of integers are the
 * same bytes in any order.
 *
 * Outputs of a cell, n_cells = n_a * n_b entries each, each nullable:
 *     count      uint32
 *     sum        int64, 8-byte aligned; exact, so frames add up (the TERRAIN block does, on the device)
 *     sum2       uint64, 8-byte aligned; likewise
 *     mean_q     int32   m = floor(sum / count), floor division towards -inf, in quanta above h0; 0x80000000 for an
 *                        empty cell
 *     spread_q2  uint32  floor(S / count) with S = the sum of (k - m)^2 = sum2 - 2 m sum + count m^2, evaluated in
 *                        wrapping 64-bit arithmetic (the true S is below 2^64 because |k - m| <= 65534, so the wrapped
 *                        result is exact; S / count <= 65534^2 < 2^32 - 1 needs no clamp); 0xFFFFFFFF for an empty
 *                        cell.  The mean squared deviation about the floor mean: within one quantum^2 of the variance
 *     flat       uint8   1 when count >= min_count and spread_q2 <= max_spread_q2, else 0
 *
 * Sites.  W = window, 0 .. 8.  A cell (i, j) = j * n_a + i is a site when every cell (i + di, j + dj) with |di|, |dj| <= W
 * lies inside the grid, is flat and has |mean_q' - mean_q(i, j)| <= max_step_q, and `allowed` is NULL or allowed[cell]
 * != 0.  The grid does not wrap: a window that leaves the grid makes no site.  site is uint8 x n_cells.
 *
 * Cost of a site, in uint32 (it cannot wrap: weights <= 4095, n <= 64, rough_cap <= 65535):
 *     cost = w_dist * ((i - goal_i)^2 + (j - goal_j)^2) + w_rough * min(spread_q2, rough_cap)
 * A goal_i >= n_a or a goal_j >= n_b switches the distance term off.
 *
 * Candidates.  n_candidates (at most 32) records {cell, cost}: as a little-endian uint64 a record is (cost << 32) | cell,
 * the steer's candidate form.  The list holds the smallest keys among the sites, ascending; ties go to the smaller cell.
 * Slots beyond the sites hold all ones.
 *
 * Summary.  uint32 x 4: the points that took part (the sum of count modulo 2^32), the number of flat cells, the number
 * of sites, 0.
 *
 * ----------------------------------------------------------------------------------- TERRAIN (d2pc_sectors_terrain_*)
 * A landing planner judges "flat" from the last second of data, on a map that moves with the vehicle.  The terrain session
 * keeps the per-cell tables (count, sum, sum2) of the last `depth` frames on the device, each with the world cell index of
 * its grid's corner, and d2pc_sectors_terrain_update_device -- ONE launch of one block behind
 * d2pc_sectors_ground_process_device -- stores the new frame's tables, sums the window as seen from the new corner and forms
 * the GROUND block's per-cell outputs, sites, cost, candidates and summary from the window's sums.  Nothing is moved when
 * the grid scrolls: a stored table stays in its own frame-local layout and is read at a shifted index.  The sums are of
 * integers: for tables that ground calls wrote, the result is the same bytes as ONE ground call over all the window's clouds
 * whose grids were placed at the new corner.  tests/sectors_terrain_ref.py restates it in numpy and Python integers.
 *
 * State (d2pc_sectors_terrain_state: one block of device memory, little-endian; two copies save and restore a map).
 *     16 headers of 16 bytes at offset 0:  {int32 ia0, int32 jb0, float h0, uint32 seq}.  seq 0 means empty; the headers
 *     at and beyond `depth` stay zero.  Then, from byte 256, `depth` tables of slot_bytes = 20 * n_cells rounded up to a
 *     multiple of 16; table s belongs to header s and holds sum[n_cells] (int64), sum2[n_cells] (uint64), count[n_cells]
 *     (uint32), in this order: the ground slab's.
 *
 * The update, from the step (the GROUND block's, the very one the ground call used: a0, b0, h0, goal_i, goal_j are read)
 * and the frame's three tables as d2pc_sectors_ground_process_device wrote them.
 *     1. Anchor.  ua = fl(a0 * inv_c), ub = fl(b0 * inv_c).  The frame is anchored iff |ua| <= 536870912.0f and |ub| <=
 *        536870912.0f, compared in float (a NaN fails).  ia0 = (int)rintf(ua), jb0 = (int)rintf(ub), half to even.  The
 *        caller keeps the corner on a multiple of the cell size.
 *     2. Not anchored: the state is untouched; every per-cell output is that of an empty window (count, sum, sum2 0, mean_q
 *        0x80000000, spread_q2 0xFFFFFFFF, flat 0, site 0), the candidates are all ones, the summary is zeros and
 *        status = {the largest seq of headers 0 .. depth - 1, 0, 0, 0}.
 *     3. Anchored.  The replaced slot v is the one with the smallest seq among slots 0 .. depth - 1, the lowest index on a
 *        tie; q = the largest seq + 1.  If the largest seq is 0xFFFFFFFF all slots are first taken as empty: v = 0, q = 1,
 *        and the headers 1 .. depth - 1 are stored as zeros.  Slot v becomes {ia0, jb0, h0, q} and a copy of the frame's
 *        three tables.
 *     4. Window of cell (i, j): the frame's entry at (i, j), always; plus, for every other slot s with seq != 0 and h0_s ==
 *        h0 (float ==: +0.0 equals -0.0, a NaN matches nothing), its entry at (i + ia0 - ia0_s, j + jb0 - jb0_s) where that
 *        lies inside the grid (the differences are formed in 64 bits).  count adds modulo 2^32, sum and sum2 modulo 2^64:
 *        exactness is the ground's as long as the window holds fewer than 2^32 points.
 *     5. mean_q, spread_q2, flat, the sites, the cost (the goal cell is relative to the current corner), the candidates and
 *        the summary are the GROUND block's, word for word, applied to the window's count, sum and sum2; min_count,
 *        max_spread_q2, max_step_q, window, the weights and rough_cap of the ground configuration now judge the WINDOW's
 *        cells.
 *     6. status = {q, the slots that took part (the frame included), (uint32)ia0, (uint32)jb0}.
 *     7. The guarantee holds for tables that ground calls wrote.  For other tables the per-cell outputs follow the wrapping
 *        formulas, and site / candidates are unspecified.
 *
 * --------------------------------------------------------------------------------------- SLOPE (d2pc_sectors_slope_*)
 * The ground judges a cell by spread_q2 alone, and a smooth 15 degree slope spreads a 0.5 m cell by 3.9 cm: as much as a
 * level cell full of rubble.  The slope session fits ONE plane per cell, k ~ c0 + gu u + gw w, so a planner reads how steep
 * a cell is (slope_a, slope_b: which way it falls), and how rough it is about its own plane (resid_q2).  It takes the
 * ground's configuration unchanged and a d2pc_sectors_slope_config beside it; d2pc_sectors_slope_process_device makes the
 * grid in at most three launches.  Every accumulated value is an integer, and the fit is one fixed sequence of double
 * operations per cell, each rounded once: the result is the same bytes whatever order the device visits the points in.
 * tests/sectors_slope_ref.py restates it in numpy.
 *
 * Configuration (d2pc_sectors_slope_config):  sub = P, the in-cell position steps per axis, 2, 4, 8 or 16;  max_slope, a
 * float, rise over run, finite and >= 0.  The host forms, in double,
 *     max_tilt2 = (double)max_slope * (double)max_slope        scale = (double)quantum * (2 * P) / (double)cell_size
 * (scale = fl(fl((double)quantum * (double)(2 * P)) / (double)cell_size): a slope in quanta per half sub-step times scale is
 * rise over run).
 *
 * Per record.  Steps 1 .. 8 of the GROUND block, word for word: the same step of 80 bytes, the same gate, cell and k.  Then
 *     9. fa = fl(va - floorf(va)),  pa = (int)floorf(fl(fa * P)),  u = 2 pa - (P - 1);  w likewise from vb.  Both float
 *        operations are exact (va < 64 and P is a power of two), so u and w are odd integers in [-(P - 1), P - 1]: the
 *        position in the cell in half sub-steps from its centre.
 *
 * Cell.  The ground's count, sum and sum2, and seven more sums over the same points, all int64:
 *     su = sum u   sw = sum w   suu = sum u^2   suw = sum u w   sww = sum w^2   suk = sum u k   swk = sum w k
 * Every term is below 2^19 in magnitude: exact for any call of fewer than 2^32 positions, the same bytes in any order.
 *
 * Fit, once per cell with count > 0.  First in wrapping 64-bit integers: m and S are the ground's floor mean and its S;
 *     r = sum - count m        suk' = suk - m su        swk' = swk - m sw
 * Then count (N), su, sw, suu, suw, sww, suk', swk', r (as int64) and S (as uint64) are converted to double, round to
 * nearest even (exact below 2^53: cells of fewer than 2^23 points).  Then, every operation in double and rounded once,
 * nothing contracted, each product of a difference rounded before the subtraction:
 *     A = N suu - su su     B = N suw - su sw     C = N sww - sw sw
 *     E = N suk' - su r     F = N swk' - sw r     G = N S - r r
 *     D = A C - B B
 *     fitted  =  count >= max(min_count, 3)  and  A C > 0  and  D * 1048576.0 > A C
 *     gu = (E C - F B) / D          gw = (F A - E B) / D
 *     Q  = (G - gu E) - gw F        c0 = ((r - gu su) - gw sw) / N
 * The third test of `fitted` refuses collinear and near-collinear point sets: it asks 1 - rho^2 > 2^-20, far above what
 * rounding can fake.
 *
 * Outputs, n_cells entries each, each nullable, at least one given:
 *     count, sum, sum2   the ground's bytes: a terrain session can still be fed
 *     moments    int64 x 7 x n_cells, 8-byte aligned: su, sw, suu, suw, sww, suk, swk, plane after plane (moments[p * n_cells
 *                + cell]).  A caller adds them across frames
 *     slope_a    float32  (float)(gu * scale): the rise along a per unit of run;  slope_b likewise from gw.  A cell that is
 *                not fitted gets the quiet NaN of bits 0x7FC00000
 *     level_q    int32    fitted: m + (int)rint(c0), half to even -- the plane at the cell's centre (rint(c0) is clamped to
 *                [-2^31, 2^31 - 1] before the conversion and the sum wraps in 32 bits; no flat cell comes near).  A cell
 *                that has points but is not fitted: m.  An empty cell: 0x80000000
 *     resid_q2   uint32   fitted: floor(max(Q, 0) / (N N)), 0xFFFFFFFE from 4294967294.0 on -- the mean squared residual
 *                about the plane (N N is one rounded product).  Points but not fitted: the ground's spread_q2.  Empty:
 *                0xFFFFFFFF
 *     flat       uint8    1 when the cell is fitted, resid_q2 <= max_spread_q2 and sa sa + sb sb <= max_tilt2 in double,
 *                sa = gu * scale, sb = gw * scale
 *     site, candidates, summary   the GROUND block's, word for word, with level_q for mean_q, resid_q2 for spread_q2 and
 *                this flat for the ground's; summary word 3 is the number of fitted cells
 *
 * ------------------------------------------------------------------------------------- RELIEF (d2pc_sectors_relief_*)
 * The terrain remembers and scrolls, but judges a cell by spread_q2 alone; the slope tells a tilted cell from a rough one,
 * but sees one call's clouds only, and a cell that a frame covers with a sliver is not fitted and is lost at the next frame.
 * The relief session is the two joined: it keeps the slope's per-cell tables (count and the nine 64-bit sums) of the last
 * `depth` frames on the device, each with the world cell index of its grid's corner, and
 * d2pc_sectors_relief_update_device -- two launches behind d2pc_sectors_slope_process_device -- stores the new frame's
 * tables, sums the window as seen from the new corner and forms the SLOPE block's fit, per-cell outputs, sites, cost,
 * candidates and summary from the window's ten sums.  u and w are positions INSIDE a cell: a scroll by whole cells does not
 * change them, so a stored table is read at a shifted index and added as it is.  The sums are of integers: for tables that
 * slope calls of the same two configurations wrote, with the caller keeping the corner on a multiple of the cell size, the
 * result is the same bytes as ONE slope call over all the window's clouds.  It takes the ground's and the slope's
 * configurations unchanged and the terrain's d2pc_sectors_terrain_config (depth) beside them.
 * tests/sectors_relief_ref.py restates it in numpy and Python integers.
 *
 * State (d2pc_sectors_relief_state: one block of device memory, little-endian; two copies save and restore a map).
 *     16 headers of 16 bytes at offset 0, exactly the terrain's:  {int32 ia0, int32 jb0, float h0, uint32 seq}.  seq 0 means
 *     empty; the headers at and beyond `depth` stay zero.  Then, from byte 256, `depth` tables of slot_bytes = 76 * n_cells
 *     rounded up to a multiple of 16; table s belongs to header s and holds nine 64-bit planes of n_cells entries each --
 *     sum, sum2, su, sw, suu, suw, sww, suk, swk, in this order -- and then count[n_cells] (uint32): the slope slab's layout.
 *
 * The update, from the step (the very one the slope call used: a0, b0, h0, goal_i, goal_j are read) and the frame's count,
 * sum, sum2 and moments (su .. swk, plane after plane) as d2pc_sectors_slope_process_device wrote them.
 *     1 .. 4 and 6.  Steps 1, 2, 3, 4 and 6 of the TERRAIN block, word for word, with the ten sums in place of the three:
 *        the anchor at 2^29 and half to even; a frame that is not anchored leaves the state untouched; the replaced slot v,
 *        q and the restart at 0xFFFFFFFF; slot v becomes {ia0, jb0, h0, q} and a copy of the frame's ten tables (sum, sum2
 *        and the seven moments into the nine planes in the order above, then count); the window of cell (i, j) is the
 *        frame's entry plus the entry at (i + ia0 - ia0_s, j + jb0 - jb0_s) of every other slot s with seq != 0 and h0_s ==
 *        h0 (float ==), where that lies inside the grid, the differences formed in 64 bits; count adds modulo 2^32, each
 *        of the nine 64-bit sums modulo 2^64; status = {q, the slots that took part (the frame included), (uint32)ia0,
 *        (uint32)jb0}.
 *     5. Every output but status is the SLOPE block's "Fit", "Outputs" and its sites, cost, candidates and summary, word
 *        for word, applied to the window's count and nine sums: count, sum, sum2 and moments are the window's; min_count,
 *        max_spread_q2, max_slope, max_step_q, window, the weights and rough_cap now judge the WINDOW's cells; the goal
 *        cell is relative to the current corner; summary word 3 is the number of fitted window cells.
 *     Not anchored: every per-cell output is that of an empty window (count, sum, sum2 and moments 0, slope_a and slope_b
 *     0x7FC00000, level_q 0x80000000, resid_q2 0xFFFFFFFF, flat 0, site 0), the candidates are all ones, the summary is
 *     zeros and status = {the largest seq of headers 0 .. depth - 1, 0, 0, 0}.
 *     The guarantee holds for tables that slope calls wrote.  For other tables the per-cell outputs follow the wrapping
 *     formulas and the fit's double sequence, and site / candidates are unspecified.
 */
#ifndef D2PC_SECTORS_H
#define D2PC_SECTORS_H

#include "d2pc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D2PC_SECTORS_MAX_SECTORS 360
#define D2PC_SECTORS_MAX_LAYERS 16
#define D2PC_SECTORS_MAX_ELEVATION_LAYERS 64   /* with n_sectors * n_layers <= 360 * 16 */
#define D2PC_SECTORS_LAYERS_HEIGHT 0      /* layer_kind: height slabs, horizontal range (the default) */
#define D2PC_SECTORS_LAYERS_ELEVATION 1   /* layer_kind: elevation-angle layers, Euclidean range */
#define D2PC_SECTORS_SHARE_POINTS 1024   /* records one block takes per step of its walk */

typedef struct d2pc_sectors_config {   /* fixed for a session */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_config) */
  int32_t device_id;
  int32_t n_sectors;           /* even, 2 .. D2PC_SECTORS_MAX_SECTORS */
  int32_t n_layers;            /* 1 .. D2PC_SECTORS_MAX_LAYERS height slabs between u_min and u_max; elevation mode:
                                  1 .. D2PC_SECTORS_MAX_ELEVATION_LAYERS layers, n_sectors * n_layers <= 5,760 */
  double azimuth0;             /* radians, finite: where sector 0 begins, from f towards l */
  float r_min, r_max;          /* range gate (horizontal; Euclidean in elevation mode), 0 <= r_min <= r_max; r_max may be +inf */
  float u_min, u_max;          /* height gate u_min <= u < u_max; -inf / +inf for none when n_layers = 1.  Elevation mode:
                                  the elevation band in radians, -1.5707964f <= u_min < u_max <= 1.5707964f */
  int32_t axes[3];             /* f, l, u: +-1, +-2, +-3 of distinct magnitudes */
  int32_t min_count;           /* >= 1: cells with fewer points report no obstacle in range / distance_cm */
  uint32_t no_obstacle_cm;     /* <= 65535: distance_cm of such a cell */
  int32_t layer_kind;          /* D2PC_SECTORS_LAYERS_HEIGHT (0, the default) or D2PC_SECTORS_LAYERS_ELEVATION */
  int32_t reserved[3];         /* zero */
} d2pc_sectors_config;
/* 72 x 1, azimuth0 = -pi/72 (sector 0 centred on forward), r 0.2 .. +inf, u -inf .. +inf, axes {3, -1, -2} (a camera's
 * optical frame, counter-clockwise), min_count 1, no_obstacle_cm 65535, device 0, height layers. */
void d2pc_sectors_config_init(d2pc_sectors_config *cfg);

typedef struct d2pc_sectors_geometry_t {
  int32_t n_cells;             /* n_sectors * n_layers: entries of every output */
  int32_t table_entries;       /* n_sectors / 2 */
  float rmin2, rmax2, inv_h;   /* as the specification forms them; inv_h is 0 when n_layers = 1 and in elevation mode */
  int32_t share_points;        /* D2PC_SECTORS_SHARE_POINTS */
  int32_t blocks_per_cu;       /* blocks of the reducing kernel per compute unit: as many as the tables in LDS allow, 4
                                  at the most; a session holds blocks_per_cu x the device's compute units of them */
  int32_t elevation_entries;   /* n_layers + 1 in elevation mode, otherwise 0 */
  size_t lds_bytes;            /* of one block: the cells' keys and counts, the boundary table and, behind it, the
                                  elevation table */
  size_t block_bytes;          /* device memory the session holds PER BLOCK (its slab of partial cells); the session
                                  adds the two tables, 8 * (table_entries + elevation_entries) bytes */
  size_t device_bytes;         /* what a session holds on an MI355X (256 compute units) */
  int32_t reserved[4];
} d2pc_sectors_geometry_t;
/* Host arithmetic only, no device.  The refusals are d2pc_sectors_create's.  D2PC_ERR_INVALID_ARG: NULL, struct_size,
 * axes, an odd n_sectors or one out of range, a NaN parameter or a non-finite azimuth0, r_min < 0, r_min > r_max,
 * u_min > u_max, min_count < 1, no_obstacle_cm > 65535, a layer_kind that is none.  D2PC_ERR_BAD_SIZE: n_layers out of
 * range; n_layers > 1 with a non-finite or empty height band, or one so narrow or wide that inv_h is not a positive
 * finite number; in elevation mode n_sectors * n_layers > 5,760, a band bound outside +-1.5707964f, u_min == u_max. */
int d2pc_sectors_geometry(const d2pc_sectors_config *cfg, d2pc_sectors_geometry_t *out);
/* Host only: the boundary table, c[j] and s[j] for j < n_sectors / 2.  Returns the number of entries (> 0), or the
 * negated d2pc_status: of the configuration's refusal, D2PC_ERR_INVALID_ARG for NULL, D2PC_ERR_CAPACITY when
 * capacity < n_sectors / 2. */
int d2pc_sectors_table(const d2pc_sectors_config *cfg, float *c, float *s, int capacity);
/* Host only: the elevation table, c[i] = ce_i and s[i] = se_i for i <= n_layers.  Returns n_layers + 1 or the negated
 * d2pc_status as d2pc_sectors_table does; D2PC_ERR_INVALID_ARG for a configuration of height layers (it has none). */
int d2pc_sectors_elevation_table(const d2pc_sectors_config *cfg, float *c, float *s, int capacity);

typedef struct d2pc_sectors d2pc_sectors;
/* Allocates everything the session will ever need (the tables and the blocks' slabs): d2pc_sectors_process_device
 * allocates nothing.  D2PC_ERR_NO_DEVICE without a GPU or for a device_id that is none. */
int d2pc_sectors_create(const d2pc_sectors_config *cfg, d2pc_sectors **out);
int d2pc_sectors_destroy(d2pc_sectors *s);
/* The message of the session's last refusal or failure ("null session" for NULL). */
const char *d2pc_sectors_last_error(const d2pc_sectors *s);
/* Blocks of the reducing kernel this session launches (0 for NULL); one block walks D2PC_SECTORS_SHARE_POINTS records
 * per step, block b takes shares b, b + blocks, ... of the call's records. */
int d2pc_sectors_blocks(const d2pc_sectors *s);

/* The clouds follow d2pc_texture_desc, so every producer plugs in unchanged. */
typedef struct d2pc_sectors_desc {
  uint32_t struct_size;        /* sizeof(d2pc_sectors_desc) */
  int32_t point_step;          /* 16 (d2pc_process_device, the rig) or 32 (d2pc_texture_device): bytes of a record */
  int32_t n_clouds;            /* 1 .. 65,535 */
  int32_t reserved;            /* zero */
  const void *points;          /* DEVICE: the records, 16-byte aligned; x, y, z are a record's first three floats */
  const uint32_t *counts;      /* DEVICE, nullable: records of each cloud (for a rig pass d_offsets + n_cameras with
                                  n_clouds 1).  NULL = cloud_points each; a count above cloud_points is clamped;
                                  0xFFFFFFFF (the in-band failure mark of d2pc_process_device) counts as 0 */
  size_t cloud_points;         /* records one cloud may hold, 1 .. 2^32 - 1 */
  size_t points_frame_stride_points;  /* records between the clouds in `points` (ignored for one cloud) */
  float *range;                /* DEVICE out, nullable; at least one of the four is given */
  uint32_t *count;
  uint32_t *nearest;
  uint16_t *distance_cm;
} d2pc_sectors_desc;
/* struct_size, point_step 16, n_clouds 1; everything else zero. */
void d2pc_sectors_desc_init(d2pc_sectors_desc *desc);
/* Host only: what d2pc_sectors_process_device refuses of `desc` for a session of `cfg`, without a session.
 * D2PC_ERR_INVALID_ARG: NULL, struct_size, point_step, n_clouds, a NULL `points`, no output, `points` not 16-byte
 * aligned, counts / an output not aligned to its type, an output that overlaps `points`, `counts` or another output.
 * D2PC_ERR_BAD_SIZE: cloud_points of 0 or >= 2^32, a frame stride below cloud_points, a largest position
 * (n_clouds - 1) * stride + cloud_points - 1 at or above 0xFFFFFFFF (that word marks an empty cell). */
int d2pc_sectors_desc_check(const d2pc_sectors_config *cfg, const d2pc_sectors_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream): two launches, no memset, no allocation, no count read on
 * the host -- it can be captured into a graph as it is, behind its producer.  Every refusal is made before anything
 * is enqueued.  The result is bit-reproducible: no float is summed and every minimum is of integers.
 * The slabs belong to the session: one launch of a session in flight per stream order; two streams need two sessions.
 */
int d2pc_sectors_process_device(d2pc_sectors *s, const d2pc_sectors_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------------------- the memory */
typedef struct d2pc_sectors_memory_config {   /* fixed for a memory session, beside the grid's d2pc_sectors_config */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_memory_config) */
  uint32_t max_age;            /* <= 0xFFFFFFFE, in the caller's ticks (say milliseconds): a record older than this is dropped */
  uint32_t reserved[2];        /* zero */
} d2pc_sectors_memory_config;

typedef struct d2pc_sectors_memory_step {   /* 64 bytes in DEVICE memory: a captured graph replays with a new pose after one small copy */
  float R[9];                  /* row-major: world = R p + t for a point p in the frame of `points` */
  float t[3];
  uint32_t dt;                 /* ticks since the previous update */
  uint32_t reserved[3];
} d2pc_sectors_memory_step;

typedef struct d2pc_sectors_fov {   /* radians; yaw from f towards l, as azimuth0 is; pitch from the horizontal plane towards u */
  double yaw, pitch, h_fov, v_fov, margin;
} d2pc_sectors_fov;

typedef struct d2pc_sectors_memory d2pc_sectors_memory;
/* Takes the grid's configuration (either layer kind) and refuses what d2pc_sectors_create refuses, with its statuses;
 * then D2PC_ERR_INVALID_ARG for a NULL or wrongly sized `mcfg` or a max_age of 0xFFFFFFFF.  Allocates everything once
 * (two record buffers of n_cells x 16 bytes, a parity word, the tables) and leaves the memory empty. */
int d2pc_sectors_memory_create(const d2pc_sectors_config *grid, const d2pc_sectors_memory_config *mcfg, d2pc_sectors_memory **out);
int d2pc_sectors_memory_destroy(d2pc_sectors_memory *m);
/* The message of the session's last refusal or failure ("null session" for NULL). */
const char *d2pc_sectors_memory_last_error(const d2pc_sectors_memory *m);

typedef struct d2pc_sectors_memory_desc {
  uint32_t struct_size;        /* sizeof(d2pc_sectors_memory_desc) */
  int32_t point_step;          /* 16 or 32, as d2pc_sectors_desc */
  int32_t n_clouds;            /* 1 .. 65,535 */
  int32_t reserved;            /* zero */
  const void *points;          /* DEVICE: the records the sectors call read, 16-byte aligned */
  size_t cloud_points;         /* as d2pc_sectors_desc: they give the position bound */
  size_t points_frame_stride_points;
  const uint32_t *count;       /* DEVICE: as d2pc_sectors_process_device wrote them for these points and this grid */
  const uint32_t *nearest;     /* DEVICE: likewise */
  const d2pc_sectors_memory_step *step;   /* DEVICE, 4-byte aligned */
  const uint8_t *covered;      /* DEVICE, nullable: one byte per cell, nonzero = the cameras look there now (a remembered
                                  point that re-bins into such a cell is dropped) */
  float *range;                /* DEVICE out, nullable; at least one of the four is given */
  uint16_t *distance_cm;
  uint32_t *age;               /* the record's age word: 0 for a fresh cell, 0xFFFFFFFF for an empty one */
  void *records;               /* n_cells x 16 bytes (world x, y, z as float32, age as uint32), 16-byte aligned */
} d2pc_sectors_memory_desc;
/* struct_size, point_step 16, n_clouds 1; everything else zero. */
void d2pc_sectors_memory_desc_init(d2pc_sectors_memory_desc *desc);
/* Host only: what d2pc_sectors_memory_update_device refuses of `desc`, without a session; first the refusals of `grid`
 * and `mcfg` as d2pc_sectors_memory_create makes them.  D2PC_ERR_INVALID_ARG: NULL, struct_size, point_step, n_clouds,
 * a NULL points / count / nearest / step, no output, points or records not 16-byte aligned, another pointer not
 * aligned to its type, an output that overlaps points, count, nearest, step, covered or another output.
 * D2PC_ERR_BAD_SIZE: cloud_points, the frame stride and the largest position as d2pc_sectors_desc_check refuses them. */
int d2pc_sectors_memory_desc_check(const d2pc_sectors_config *grid, const d2pc_sectors_memory_config *mcfg,
                                   const d2pc_sectors_memory_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream): ONE launch of one block, no memset, no allocation, no host
 * read -- it can be captured into a graph behind d2pc_sectors_process_device.  Every refusal is made before anything is
 * enqueued.  The session holds two record buffers and a parity word in device memory: the launch reads one buffer,
 * writes the other and flips the word last, on the device, so a replayed graph advances the memory as plain calls do.
 * Bit-reproducible: every minimum is of integers.  One update of a session in flight per stream order.
 */
int d2pc_sectors_memory_update_device(d2pc_sectors_memory *m, const d2pc_sectors_memory_desc *desc, void *stream);
/* Asynchronous: empties the memory with one launch (no memset node). */
int d2pc_sectors_memory_reset_device(d2pc_sectors_memory *m, void *stream);
/*
 * Host only: which cells the cameras look at, for `covered`.  A cell is covered when its centre direction passes, for
 * some FOV, in double:  |wrap(az_c - yaw)| <= h_fov / 2 - margin  and, for elevation layers,
 * |el_c - pitch| <= v_fov / 2 - margin;  az_c = azimuth0 + 2 pi (k + 1/2) / n_sectors,  el_c = (e_i + e_{i+1}) / 2,
 * wrap(x) = the IEEE remainder of x by 2 pi.  Height layers: the azimuth test alone, every layer alike.
 * Writes n_cells bytes (1 or 0) and returns n_cells, or the negated d2pc_status: of the configuration's refusal,
 * D2PC_ERR_INVALID_ARG for a NULL `covered_host`, n_fovs < 0 or NULL `fovs` with n_fovs > 0, D2PC_ERR_CAPACITY when
 * capacity < n_cells.
 */
int d2pc_sectors_memory_coverage(const d2pc_sectors_config *grid, const d2pc_sectors_fov *fovs, int n_fovs,
                                 uint8_t *covered_host, int capacity);

/* -------------------------------------------------------------------------------------------------------- the steer */
#define D2PC_SECTORS_STEER_MAX_REACH_SECTORS 32
#define D2PC_SECTORS_STEER_MAX_REACH_LAYERS 16
#define D2PC_SECTORS_STEER_MAX_CANDIDATES 32
#define D2PC_SECTORS_STEER_MAX_WEIGHT 4095
#define D2PC_SECTORS_STEER_OFF 0xFFFFFFFFu   /* a goal_sector / prev_sector that switches its term off (any value >= n_sectors does) */

typedef struct d2pc_sectors_steer_config {   /* fixed for a steer session, beside the grid's d2pc_sectors_config */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_steer_config) */
  float radius;                /* the vehicle's radius plus margin, in the cloud's unit (metres); finite and > 0 */
  int32_t max_reach_sectors;   /* Wa: 0 .. 32 and <= n_sectors / 2 */
  int32_t max_reach_layers;    /* We: 0 .. 16 and <= n_layers - 1 */
  uint32_t free_cm;            /* <= 65535: a distance_cm at or above it is nothing there */
  uint32_t min_clearance_cm;   /* <= 65535: a cell is free from this clearance on */
  uint32_t horizon_cm;         /* <= 65535: clearance beyond it costs nothing */
  uint32_t w_goal, w_prev, w_near;   /* <= 4095 each */
  uint32_t reserved[2];        /* zero */
} d2pc_sectors_steer_config;
/* radius 0.5, reach 8 sectors / 0 layers, free_cm 65535, min_clearance_cm 100, horizon_cm 1000, weights 16 / 4 / 1. */
void d2pc_sectors_steer_config_init(d2pc_sectors_steer_config *scfg);

typedef struct d2pc_sectors_steer_step {   /* 32 bytes in DEVICE memory: a captured graph replays with a new goal after one small copy */
  uint32_t goal_sector, goal_layer;   /* a sector >= n_sectors switches the term off; a layer >= n_layers is n_layers - 1 */
  uint32_t prev_sector, prev_layer;   /* the previous heading, likewise */
  uint32_t reserved[4];
} d2pc_sectors_steer_step;

typedef struct d2pc_sectors_steer_candidate {   /* as a little-endian uint64: (cost << 32) | cell */
  uint32_t cell, cost;
} d2pc_sectors_steer_candidate;

/* Host only: the reach tables.  reach_sectors gets n_layers x (Wa + 1) entries, row i = reach_s[i][0 .. Wa];
 * reach_layers gets We + 1.  Returns the entries of reach_sectors (reach_layers' are max_reach_layers + 1), or the
 * negated d2pc_status: of the refusal of `grid` or `scfg` as d2pc_sectors_steer_desc_check makes them,
 * D2PC_ERR_INVALID_ARG for a NULL table, D2PC_ERR_CAPACITY when a capacity (in entries) is too small. */
int d2pc_sectors_steer_reach(const d2pc_sectors_config *grid, const d2pc_sectors_steer_config *scfg, uint16_t *reach_sectors,
                             int sectors_capacity, uint16_t *reach_layers, int layers_capacity);
/* Host only, in double: the cell of a direction, for a step.  sector = floor(wrap(yaw - azimuth0) / alpha) with wrap
 * into [0, 2 pi).  Elevation layers: the layer is the number of i in 1 .. n_layers - 1 with pitch >= e_i;
 * D2PC_ERR_INVALID_ARG for a pitch outside [e_0, e_L).  Height layers: the third argument is the layer itself, floored;
 * D2PC_ERR_INVALID_ARG outside [0, n_layers).  D2PC_ERR_INVALID_ARG also for NULL or a direction that is not finite. */
int d2pc_sectors_steer_goal_cell(const d2pc_sectors_config *grid, double yaw, double pitch_or_layer, uint32_t *sector,
                                 uint32_t *layer);

typedef struct d2pc_sectors_steer d2pc_sectors_steer;
/* Refuses what d2pc_sectors_steer_desc_check refuses of `grid` and `scfg`.  Allocates the two reach tables on the device
 * and nothing else, ever.  D2PC_ERR_NO_DEVICE without a GPU or for a device_id that is none. */
int d2pc_sectors_steer_create(const d2pc_sectors_config *grid, const d2pc_sectors_steer_config *scfg, d2pc_sectors_steer **out);
int d2pc_sectors_steer_destroy(d2pc_sectors_steer *s);
/* The message of the session's last refusal or failure ("null session" for NULL). */
const char *d2pc_sectors_steer_last_error(const d2pc_sectors_steer *s);

typedef struct d2pc_sectors_steer_desc {
  uint32_t struct_size;        /* sizeof(d2pc_sectors_steer_desc) */
  int32_t n_candidates;        /* 1 .. 32 when `candidates` is given */
  const uint16_t *distance_cm; /* DEVICE: n_cells, as d2pc_sectors_process_device or d2pc_sectors_memory_update_device wrote them */
  const uint8_t *allowed;      /* DEVICE, nullable: one byte per cell, zero = not to be steered into (d2pc_sectors_memory_coverage
                                  makes such a mask) */
  const d2pc_sectors_steer_step *step;   /* DEVICE, 4-byte aligned */
  uint16_t *clearance_cm;      /* DEVICE out, nullable; at least one of the four is given */
  uint32_t *cost;
  d2pc_sectors_steer_candidate *candidates;   /* n_candidates records, 8-byte aligned */
  uint32_t *summary;           /* 4 words */
} d2pc_sectors_steer_desc;
/* struct_size, n_candidates 1; everything else zero. */
void d2pc_sectors_steer_desc_init(d2pc_sectors_steer_desc *desc);
/* Host only: what d2pc_sectors_steer_device refuses, without a session.  First the refusals of `grid` with the grid's
 * statuses, then the steer configuration's -- D2PC_ERR_INVALID_ARG: NULL, struct_size, a radius that is NaN, zero, negative
 * or not finite, a weight > 4095, a *_cm > 65535; D2PC_ERR_BAD_SIZE: a reach that is negative or above its cap,
 * max_reach_sectors > n_sectors / 2, max_reach_layers > n_layers - 1 (or > 0 without a finite height band) -- then the
 * descriptor's, all D2PC_ERR_INVALID_ARG: NULL, struct_size, a NULL distance_cm or step, no output, n_candidates out of
 * 1 .. 32 when candidates is given, a pointer not aligned to its type (8 bytes for candidates), an output that overlaps
 * distance_cm, allowed, step or another output. */
int d2pc_sectors_steer_desc_check(const d2pc_sectors_config *grid, const d2pc_sectors_steer_config *scfg,
                                  const d2pc_sectors_steer_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream): ONE launch of one block, no memset, no allocation, no host
 * read -- it can be captured into a graph behind d2pc_sectors_process_device or d2pc_sectors_memory_update_device.  Every
 * refusal is made before anything is enqueued.  Bit-reproducible: every value is an integer and every minimum is of
 * distinct keys.  The session holds nothing the launch writes: calls of one session may be in flight on several streams.
 */
int d2pc_sectors_steer_device(d2pc_sectors_steer *s, const d2pc_sectors_steer_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------------------- the ground */
#define D2PC_SECTORS_GROUND_MAX_CELLS_PER_AXIS 64
#define D2PC_SECTORS_GROUND_MAX_WINDOW 8
#define D2PC_SECTORS_GROUND_MAX_CANDIDATES 32
#define D2PC_SECTORS_GROUND_MAX_WEIGHT 4095
#define D2PC_SECTORS_GROUND_MAX_K 32767             /* |k| of a point that takes part */
#define D2PC_SECTORS_GROUND_EMPTY_MEAN 0x80000000u  /* mean_q of an empty cell, as a uint32 */
#define D2PC_SECTORS_GROUND_EMPTY_SPREAD 0xFFFFFFFFu
#define D2PC_SECTORS_GROUND_OFF 0xFFFFFFFFu         /* a goal_i / goal_j that switches the distance term off (any value >= n does) */

typedef struct d2pc_sectors_ground_config {   /* fixed for a ground session */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_ground_config) */
  int32_t device_id;
  int32_t n_a, n_b;            /* 2 .. 64 each: cells along a and along b */
  float cell_size;             /* finite and > 0, in the cloud's unit (metres) */
  float quantum;               /* finite and > 0: the height of one k */
  int32_t axes[3];             /* a, b, h picked from the WORLD point: +-1, +-2, +-3 of distinct magnitudes */
  uint32_t min_count;          /* >= 1: a cell with fewer points is not flat */
  uint32_t max_spread_q2;      /* a cell with a larger spread_q2 is not flat (d2pc_sectors_ground_spread_of_std makes it) */
  uint32_t max_step_q;         /* <= 65535: the largest |mean_q' - mean_q| inside a site's window */
  int32_t window;              /* W: 0 .. 8 */
  uint32_t w_dist, w_rough;    /* <= 4095 each */
  uint32_t rough_cap;          /* <= 65535 */
  uint32_t max_points;         /* the records of the largest call the session is meant for: it sizes the reducing blocks;
                                  0 = size by the device.  A larger call stays correct: blocks walk more shares */
  uint32_t reserved[3];        /* zero */
} d2pc_sectors_ground_config;
/* 16 x 16 cells of 0.5, quantum 0.002, axes {1, 2, 3} (ENU), min_count 4, max_spread_q2 625 (a standard deviation of
 * 0.05), max_step_q 50 (0.1), window 1, w_dist 1, w_rough 1, rough_cap 65535, max_points 0, device 0. */
void d2pc_sectors_ground_config_init(d2pc_sectors_ground_config *gcfg);

typedef struct d2pc_sectors_ground_geometry_t {
  int32_t n_cells;             /* n_a * n_b: entries of every per-cell output */
  float inv_c, inv_q;          /* as the specification forms them */
  int32_t share_points;        /* D2PC_SECTORS_SHARE_POINTS */
  int32_t blocks_per_cu;       /* reducing blocks per compute unit: as many as 160 KiB of LDS hold, 4 at the most */
  int32_t blocks;              /* reducing blocks of a session on an MI355X (256 compute units): one per 4 shares of
                                  max_points, 1 .. blocks_per_cu x compute units; all of them for max_points 0 */
  size_t lds_bytes;            /* of one reducing block: 20 bytes per cell */
  size_t block_bytes;          /* device memory the session holds PER BLOCK: its slab of partial cells, 20 bytes per cell,
                                  rounded up to a multiple of 8 for an odd n_cells (5 x 3 cells: 304, not 300) */
  size_t device_bytes;         /* what a session holds on an MI355X: the slabs and 13 bytes per cell between the launches */
  int32_t reserved[4];
} d2pc_sectors_ground_geometry_t;
/* Host arithmetic only, no device.  The refusals are d2pc_sectors_ground_create's.  D2PC_ERR_INVALID_ARG: NULL,
 * struct_size, axes, a cell_size or quantum that is NaN, not finite, zero or negative, min_count < 1, max_step_q >
 * 65535, a weight > 4095, rough_cap > 65535, a reserved word that is not zero.  D2PC_ERR_BAD_SIZE: n_a or n_b outside
 * 2 .. 64, window outside 0 .. 8, an inv_c or inv_q that is not a positive finite float. */
int d2pc_sectors_ground_geometry(const d2pc_sectors_ground_config *gcfg, d2pc_sectors_ground_geometry_t *out);
/* Host only, in double: max_spread_q2 from a standard deviation in the cloud's unit, floor((std / quantum)^2) clamped to
 * 0xFFFFFFFE.  0 for a quantum that is not finite and > 0 or a std that is NaN or negative. */
uint32_t d2pc_sectors_ground_spread_of_std(double quantum, double std_dev);

typedef struct d2pc_sectors_ground_step {   /* 80 bytes in DEVICE memory: a captured graph replays with a new pose after one small copy */
  float R[9];                  /* row-major: world = R p + t for a point p in the frame of `points` */
  float t[3];
  float origin[3];             /* a0, b0: the grid's corner; h0: the reference height */
  uint32_t goal_i, goal_j;     /* the cell the cost measures from; a goal_i >= n_a or a goal_j >= n_b switches the term off */
  uint32_t reserved[3];
} d2pc_sectors_ground_step;

typedef d2pc_sectors_steer_candidate d2pc_sectors_ground_candidate;   /* as a little-endian uint64: (cost << 32) | cell */

typedef struct d2pc_sectors_ground d2pc_sectors_ground;
/* Allocates everything the session will ever need (the blocks' slabs and 13 bytes per cell that the launches hand on).
 * D2PC_ERR_NO_DEVICE without a GPU or for a device_id that is none. */
int d2pc_sectors_ground_create(const d2pc_sectors_ground_config *gcfg, d2pc_sectors_ground **out);
int d2pc_sectors_ground_destroy(d2pc_sectors_ground *g);
/* The message of the session's last refusal or failure ("null session" for NULL). */
const char *d2pc_sectors_ground_last_error(const d2pc_sectors_ground *g);
/* Reducing blocks this session holds slabs for (0 for NULL): geometry's arithmetic with the device's compute units.  A call
 * launches min(blocks, its shares) of them. */
int d2pc_sectors_ground_blocks(const d2pc_sectors_ground *g);

typedef struct d2pc_sectors_ground_desc {   /* the clouds exactly as d2pc_sectors_desc takes them */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_ground_desc) */
  int32_t point_step;          /* 16 or 32 */
  int32_t n_clouds;            /* 1 .. 65,535 */
  int32_t n_candidates;        /* 1 .. 32 when `candidates` is given */
  const void *points;          /* DEVICE: the records, 16-byte aligned */
  const uint32_t *counts;      /* DEVICE, nullable: as d2pc_sectors_desc (clamped to cloud_points; 0xFFFFFFFF reads as 0) */
  size_t cloud_points;         /* 1 .. 2^32 - 1 */
  size_t points_frame_stride_points;
  const d2pc_sectors_ground_step *step;   /* DEVICE, 4-byte aligned */
  const uint8_t *allowed;      /* DEVICE, nullable: one byte per cell, zero = no site */
  uint32_t *count;             /* DEVICE out, each nullable; at least one of the nine is given */
  int64_t *sum;                /* 8-byte aligned */
  uint64_t *sum2;              /* 8-byte aligned */
  int32_t *mean_q;
  uint32_t *spread_q2;
  uint8_t *flat;
  uint8_t *site;
  d2pc_sectors_ground_candidate *candidates;   /* n_candidates records, 8-byte aligned */
  uint32_t *summary;           /* 4 words */
} d2pc_sectors_ground_desc;
/* struct_size, point_step 16, n_clouds 1, n_candidates 1; everything else zero. */
void d2pc_sectors_ground_desc_init(d2pc_sectors_ground_desc *desc);
/* Host only: what d2pc_sectors_ground_process_device refuses of `desc` for a session of `gcfg`, without a session; first
 * the refusals of `gcfg`.  D2PC_ERR_INVALID_ARG: NULL, struct_size, point_step, n_clouds, a NULL points or step, no output,
 * n_candidates out of 1 .. 32 when candidates is given, points not 16-byte aligned, another pointer not aligned to its type
 * (8 bytes for sum, sum2 and candidates), an output that overlaps points, counts, step, allowed or another output.
 * D2PC_ERR_BAD_SIZE: cloud_points, the frame stride and the largest position as d2pc_sectors_desc_check refuses them. */
int d2pc_sectors_ground_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_ground_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream): three launches (two when neither site, candidates nor summary
 * is asked for), no memset, no allocation, no count read on the host -- it can be captured into a graph as it is, behind
 * its producer.  Every refusal is made before anything is enqueued.  Bit-reproducible: every sum is of integers.
 * The slabs belong to the session: one call of a session in flight per stream order; two streams need two sessions.
 */
int d2pc_sectors_ground_process_device(d2pc_sectors_ground *g, const d2pc_sectors_ground_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------------------ the terrain */
#define D2PC_SECTORS_TERRAIN_MAX_DEPTH 16
#define D2PC_SECTORS_TERRAIN_HEADER_BYTES 16        /* {int32 ia0, int32 jb0, float h0, uint32 seq} */
#define D2PC_SECTORS_TERRAIN_MAX_CORNER 536870912   /* 2^29: the largest |corner| in cells that anchors a frame */

typedef struct d2pc_sectors_terrain_config {   /* fixed for a terrain session, beside the ground configuration */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_terrain_config) */
  int32_t depth;               /* 1 .. 16: the frames of the window, the newest included */
  uint32_t reserved[6];        /* zero */
} d2pc_sectors_terrain_config;
/* depth 8. */
void d2pc_sectors_terrain_config_init(d2pc_sectors_terrain_config *tcfg);

typedef struct d2pc_sectors_terrain_geometry_t {
  int32_t n_cells;             /* n_a * n_b */
  float inv_c;                 /* as the specification forms it: the anchor's factor */
  size_t slot_bytes;           /* one stored table: 20 * n_cells rounded up to a multiple of 16 */
  size_t state_bytes;          /* the state block: 256 + depth * slot_bytes */
  size_t headers_offset;       /* 0 */
  size_t tables_offset;        /* 256: table s begins at tables_offset + s * slot_bytes */
  int32_t reserved[6];
} d2pc_sectors_terrain_geometry_t;
/* Host arithmetic only, no device.  First the refusals of d2pc_sectors_ground_geometry for `gcfg`, unchanged; then, in this
 * order, D2PC_ERR_INVALID_ARG: a NULL tcfg, its struct_size;  D2PC_ERR_BAD_SIZE: depth outside 1 .. 16;
 * D2PC_ERR_INVALID_ARG: a reserved word that is not zero.  A NULL `out` is D2PC_ERR_INVALID_ARG before all of them. */
int d2pc_sectors_terrain_geometry(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_terrain_config *tcfg,
                                  d2pc_sectors_terrain_geometry_t *out);

typedef struct d2pc_sectors_terrain d2pc_sectors_terrain;
/* `gcfg` is the configuration the ground session was made from: its grid, cell_size, min_count, max_spread_q2, max_step_q,
 * window, weights and rough_cap now apply to the WINDOW's cells (quantum, axes and max_points are checked and not used).
 * Allocates the state once, with every header zero.  D2PC_ERR_NO_DEVICE without a GPU or for a device_id that is none. */
int d2pc_sectors_terrain_create(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_terrain_config *tcfg, d2pc_sectors_terrain **out);
int d2pc_sectors_terrain_destroy(d2pc_sectors_terrain *t);
/* The message of the session's last refusal or failure ("null session" for NULL). */
const char *d2pc_sectors_terrain_last_error(const d2pc_sectors_terrain *t);
/* The state block in DEVICE memory and its size (each nullable), laid out as the TERRAIN block documents: a caller saves and
 * restores a map with one copy each way, in stream order with the updates. */
int d2pc_sectors_terrain_state(const d2pc_sectors_terrain *t, void **device_ptr, size_t *bytes);
/* Asynchronous on `stream`: one small launch that zeroes the 16 headers with vector stores (the window is empty again;
 * the tables are left as they are, nothing reads a table of an empty header). */
int d2pc_sectors_terrain_reset_device(d2pc_sectors_terrain *t, void *stream);

typedef struct d2pc_sectors_terrain_desc {
  uint32_t struct_size;        /* sizeof(d2pc_sectors_terrain_desc) */
  int32_t n_candidates;        /* 1 .. 32 when `candidates` is given */
  const d2pc_sectors_ground_step *step;   /* DEVICE, 4-byte aligned: the very step the ground call used */
  const uint32_t *frame_count; /* DEVICE in, all three required: n_cells entries each, as */
  const int64_t *frame_sum;    /*   d2pc_sectors_ground_process_device wrote them (count, sum, sum2); */
  const uint64_t *frame_sum2;  /*   frame_sum and frame_sum2 8-byte aligned */
  const uint8_t *allowed;      /* DEVICE, nullable: one byte per cell, zero = no site */
  uint32_t *count;             /* DEVICE out, the WINDOW's, each nullable; at least one of these ten is given */
  int64_t *sum;                /* 8-byte aligned */
  uint64_t *sum2;              /* 8-byte aligned */
  int32_t *mean_q;
  uint32_t *spread_q2;
  uint8_t *flat;
  uint8_t *site;
  d2pc_sectors_ground_candidate *candidates;   /* n_candidates records, 8-byte aligned */
  uint32_t *summary;           /* 4 words */
  uint32_t *status;            /* 4 words: {seq, slots that took part, (uint32)ia0, (uint32)jb0} */
} d2pc_sectors_terrain_desc;
/* struct_size, n_candidates 1; everything else zero. */
void d2pc_sectors_terrain_desc_init(d2pc_sectors_terrain_desc *desc);
/* Host only: what d2pc_sectors_terrain_update_device refuses of `desc` for a session of `gcfg` and `tcfg`, without a
 * session; first the refusals of the two configurations.  D2PC_ERR_INVALID_ARG: NULL, struct_size, a NULL step, frame_count,
 * frame_sum or frame_sum2, no output, n_candidates out of 1 .. 32 when candidates is given, a pointer not aligned to its
 * type (8 bytes for frame_sum, frame_sum2, sum, sum2 and candidates), an output that overlaps step, a frame table, allowed
 * or another output.  The session adds one refusal: a buffer that overlaps its own state block. */
int d2pc_sectors_terrain_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_terrain_config *tcfg,
                                    const d2pc_sectors_terrain_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream): ONE launch of one block, no memset, no allocation, no host
 * read -- it can be captured into a graph behind d2pc_sectors_ground_process_device.  Every refusal is made before anything
 * is enqueued.  Bit-reproducible: every sum is of integers and every minimum is of distinct keys.  The state belongs to the
 * session: one update of a session in flight per stream order.
 */
int d2pc_sectors_terrain_update_device(d2pc_sectors_terrain *t, const d2pc_sectors_terrain_desc *desc, void *stream);

/* -------------------------------------------------------------------------------------------------------- the slope */
#define D2PC_SECTORS_SLOPE_CELL_BYTES 76            /* of a reducing block's table and of its slab: nine 64-bit sums and the count */
#define D2PC_SECTORS_SLOPE_MAX_CELLS 2155           /* 76 bytes per cell in the 163,840 bytes of one block's LDS */
#define D2PC_SECTORS_SLOPE_MOMENTS 7                /* planes of `moments`: su, sw, suu, suw, sww, suk, swk */
#define D2PC_SECTORS_SLOPE_NOT_FITTED 0x7FC00000u   /* slope_a / slope_b of a cell that is not fitted, as bits */

typedef struct d2pc_sectors_slope_config {   /* fixed for a slope session, beside the ground configuration */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_slope_config) */
  int32_t sub;                 /* P: 2, 4, 8 or 16 in-cell position steps per axis */
  float max_slope;             /* finite and >= 0, rise over run: a steeper cell is not flat (d2pc_sectors_slope_of_degrees makes it) */
  uint32_t reserved[5];        /* zero */
} d2pc_sectors_slope_config;
/* sub 8, max_slope 0.26794919 (15 degrees). */
void d2pc_sectors_slope_config_init(d2pc_sectors_slope_config *scfg);

typedef struct d2pc_sectors_slope_geometry_t {
  int32_t n_cells;             /* n_a * n_b: entries of every per-cell output */
  int32_t blocks_per_cu;       /* reducing blocks per compute unit: as many as 160 KiB of LDS hold, 4 at the most */
  int32_t blocks;              /* reducing blocks of a session on an MI355X: the ground's arithmetic with this blocks_per_cu */
  int32_t sub;                 /* P */
  size_t lds_bytes;            /* of one reducing block: 76 bytes per cell */
  size_t block_bytes;          /* device memory the session holds PER BLOCK: 76 bytes per cell, rounded up to a multiple of 8 */
  size_t device_bytes;         /* what a session holds on an MI355X: the slabs and 14 bytes per cell between the launches */
  double scale, max_tilt2;     /* as the specification forms them */
  int32_t reserved[4];
} d2pc_sectors_slope_geometry_t;
/* Host arithmetic only, no device.  A NULL `out` is D2PC_ERR_INVALID_ARG before everything.  First the refusals of
 * d2pc_sectors_ground_geometry for `gcfg`, unchanged; then, in this order, D2PC_ERR_INVALID_ARG: a NULL scfg or its
 * struct_size, a sub that is not 2, 4, 8 or 16, a max_slope that is NaN, not finite or negative, a reserved word that is
 * not zero;  D2PC_ERR_BAD_SIZE: n_cells * 76 > 163,840 (more than 2,155 cells: 46 x 46 and 64 x 32 pass, 64 x 64 does not). */
int d2pc_sectors_slope_geometry(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                d2pc_sectors_slope_geometry_t *out);
/* Host only, in double: max_slope from an angle, (float)tan(degrees * pi / 180).  0 for an angle that is NaN, negative or
 * 90 and more. */
float d2pc_sectors_slope_of_degrees(double degrees);

typedef struct d2pc_sectors_slope d2pc_sectors_slope;
/* Allocates everything the session will ever need (the blocks' slabs and 14 bytes per cell that the launches hand on).
 * D2PC_ERR_NO_DEVICE without a GPU or for a device_id that is none. */
int d2pc_sectors_slope_create(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg, d2pc_sectors_slope **out);
int d2pc_sectors_slope_destroy(d2pc_sectors_slope *s);
/* The message of the session's last refusal or failure ("null session" for NULL). */
const char *d2pc_sectors_slope_last_error(const d2pc_sectors_slope *s);
/* Reducing blocks this session holds slabs for (0 for NULL).  A call launches min(blocks, its shares) of them. */
int d2pc_sectors_slope_blocks(const d2pc_sectors_slope *s);

typedef struct d2pc_sectors_slope_desc {   /* d2pc_sectors_ground_desc with the slope's outputs */
  uint32_t struct_size;        /* sizeof(d2pc_sectors_slope_desc) */
  int32_t point_step;          /* 16 or 32 */
  int32_t n_clouds;            /* 1 .. 65,535 */
  int32_t n_candidates;        /* 1 .. 32 when `candidates` is given */
  const void *points;          /* DEVICE: the records, 16-byte aligned */
  const uint32_t *counts;      /* DEVICE, nullable: as d2pc_sectors_desc */
  size_t cloud_points;         /* 1 .. 2^32 - 1 */
  size_t points_frame_stride_points;
  const d2pc_sectors_ground_step *step;   /* DEVICE, 4-byte aligned */
  const uint8_t *allowed;      /* DEVICE, nullable: one byte per cell, zero = no site */
  uint32_t *count;             /* DEVICE out, each nullable; at least one of the twelve is given */
  int64_t *sum;                /* 8-byte aligned */
  uint64_t *sum2;              /* 8-byte aligned */
  int64_t *moments;            /* 7 x n_cells, 8-byte aligned */
  float *slope_a, *slope_b;
  int32_t *level_q;
  uint32_t *resid_q2;
  uint8_t *flat;
  uint8_t *site;
  d2pc_sectors_ground_candidate *candidates;   /* n_candidates records, 8-byte aligned */
  uint32_t *summary;           /* 4 words */
} d2pc_sectors_slope_desc;
/* struct_size, point_step 16, n_clouds 1, n_candidates 1; everything else zero. */
void d2pc_sectors_slope_desc_init(d2pc_sectors_slope_desc *desc);
/* Host only: what d2pc_sectors_slope_process_device refuses of `desc`, without a session; first the refusals of the two
 * configurations as d2pc_sectors_slope_geometry makes them.  Then the ground descriptor's, in its order, with the new
 * outputs beside the old: D2PC_ERR_INVALID_ARG: NULL, struct_size, point_step, n_clouds, a NULL points or step, no output,
 * n_candidates out of 1 .. 32 when candidates is given, points not 16-byte aligned, another pointer not aligned to its type
 * (8 bytes for sum, sum2, moments and candidates), an output that overlaps points, counts, step, allowed or another output.
 * D2PC_ERR_BAD_SIZE: cloud_points, the frame stride and the largest position as d2pc_sectors_desc_check refuses them. */
int d2pc_sectors_slope_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                  const d2pc_sectors_slope_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream): three launches (two when neither site, candidates nor summary
 * is asked for), no memset, no allocation, no count read on the host -- it can be captured into a graph as it is, behind
 * its producer, and replays with a new pose after one 80-byte copy into `step`.  Every refusal is made before anything is
 * enqueued.  Bit-reproducible: every sum is of integers and the fit is one fixed sequence of double operations per cell.
 * The slabs belong to the session: one call of a session in flight per stream order; two streams need two sessions.
 */
int d2pc_sectors_slope_process_device(d2pc_sectors_slope *s, const d2pc_sectors_slope_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------------------- the relief */
typedef struct d2pc_sectors_relief_geometry_t {
  int32_t n_cells;             /* n_a * n_b */
  float inv_c;                 /* as the specification forms it: the anchor's factor */
  size_t slot_bytes;           /* one stored table: 76 * n_cells rounded up to a multiple of 16 */
  size_t state_bytes;          /* the state block: 256 + depth * slot_bytes */
  size_t headers_offset;       /* 0 */
  size_t tables_offset;        /* 256: table s begins at tables_offset + s * slot_bytes */
  double scale, max_tilt2;     /* the slope's, as the specification forms them */
  int32_t blocks;              /* of the window launch: 16 cells each */
  int32_t reserved[5];
} d2pc_sectors_relief_geometry_t;
/* Host arithmetic only, no device.  A NULL `out` is D2PC_ERR_INVALID_ARG before everything.  First the refusals of
 * d2pc_sectors_slope_geometry for `gcfg` and `scfg`, unchanged and in its order (the ground's, the slope's, more than 2,155
 * cells); then those of `tcfg` as d2pc_sectors_terrain_geometry lists them: D2PC_ERR_INVALID_ARG: a NULL tcfg, its
 * struct_size;  D2PC_ERR_BAD_SIZE: depth outside 1 .. 16;  D2PC_ERR_INVALID_ARG: a reserved word that is not zero. */
int d2pc_sectors_relief_geometry(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                 const d2pc_sectors_terrain_config *tcfg, d2pc_sectors_relief_geometry_t *out);

typedef struct d2pc_sectors_relief d2pc_sectors_relief;
/* `gcfg` and `scfg` are the configurations the slope session was made from: min_count, max_spread_q2, max_slope, max_step_q,
 * window, the weights and rough_cap now apply to the WINDOW's cells.  Allocates the state once, with every header zero, and
 * 14 bytes per cell that the two launches hand on.  D2PC_ERR_NO_DEVICE without a GPU or for a device_id that is none. */
int d2pc_sectors_relief_create(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                               const d2pc_sectors_terrain_config *tcfg, d2pc_sectors_relief **out);
int d2pc_sectors_relief_destroy(d2pc_sectors_relief *r);
/* The message of the session's last refusal or failure ("null session" for NULL). */
const char *d2pc_sectors_relief_last_error(const d2pc_sectors_relief *r);
/* The state block in DEVICE memory and its size (each nullable), laid out as the RELIEF block documents: a caller saves and
 * restores a map with one copy each way, in stream order with the updates. */
int d2pc_sectors_relief_state(const d2pc_sectors_relief *r, void **device_ptr, size_t *bytes);
/* Asynchronous on `stream`: one small launch that zeroes the 16 headers with vector stores (the window is empty again;
 * the tables are left as they are, nothing reads a table of an empty header). */
int d2pc_sectors_relief_reset_device(d2pc_sectors_relief *r, void *stream);

typedef struct d2pc_sectors_relief_desc {
  uint32_t struct_size;        /* sizeof(d2pc_sectors_relief_desc) */
  int32_t n_candidates;        /* 1 .. 32 when `candidates` is given */
  const d2pc_sectors_ground_step *step;   /* DEVICE, 4-byte aligned: the very step the slope call used */
  const uint32_t *frame_count; /* DEVICE in, all four required: as d2pc_sectors_slope_process_device wrote them */
  const int64_t *frame_sum;    /*   (count, sum, sum2: n_cells entries each; moments: 7 x n_cells); */
  const uint64_t *frame_sum2;  /*   frame_sum, frame_sum2 and frame_moments 8-byte aligned */
  const int64_t *frame_moments;
  const uint8_t *allowed;      /* DEVICE, nullable: one byte per cell, zero = no site */
  uint32_t *count;             /* DEVICE out, the WINDOW's, each nullable; at least one of these thirteen is given */
  int64_t *sum;                /* 8-byte aligned */
  uint64_t *sum2;              /* 8-byte aligned */
  int64_t *moments;            /* 7 x n_cells, 8-byte aligned */
  float *slope_a, *slope_b;
  int32_t *level_q;
  uint32_t *resid_q2;
  uint8_t *flat;
  uint8_t *site;
  d2pc_sectors_ground_candidate *candidates;   /* n_candidates records, 8-byte aligned */
  uint32_t *summary;           /* 4 words */
  uint32_t *status;            /* 4 words: {seq, slots that took part, (uint32)ia0, (uint32)jb0} */
} d2pc_sectors_relief_desc;
/* struct_size, n_candidates 1; everything else zero. */
void d2pc_sectors_relief_desc_init(d2pc_sectors_relief_desc *desc);
/* Host only: what d2pc_sectors_relief_update_device refuses of `desc` for a session of the three configurations, without a
 * session; first the refusals of the configurations as d2pc_sectors_relief_geometry makes them.  D2PC_ERR_INVALID_ARG: NULL,
 * struct_size, a NULL step, frame_count, frame_sum, frame_sum2 or frame_moments, no output, n_candidates out of 1 .. 32 when
 * candidates is given, a pointer not aligned to its type (8 bytes for frame_sum, frame_sum2, frame_moments, sum, sum2,
 * moments and candidates), an output that overlaps step, a frame table, allowed or another output.  The session adds one
 * refusal: a buffer that overlaps its own state block. */
int d2pc_sectors_relief_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                   const d2pc_sectors_terrain_config *tcfg, const d2pc_sectors_relief_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream): TWO launches -- the window and the fit in many blocks, then one
 * block that commits the header, writes status and ranks the sites --, no global atomic, no memset, no allocation, no host
 * read: it can be captured into a graph behind d2pc_sectors_slope_process_device.  Every refusal is made before anything is
 * enqueued.  Bit-reproducible: every sum is of integers, the fit is one fixed sequence of double operations per cell and
 * every minimum is of distinct keys.  The state belongs to the session: one update of a session in flight per stream order.
 */
int d2pc_sectors_relief_update_device(d2pc_sectors_relief *r, const d2pc_sectors_relief_desc *desc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D2PC_SECTORS_H */
