"""Demand variants: other trips on the same scenario, one variant per environment of a batch (BatchedSim.set_demand).

The reference varies demand per run: MultiSignal(route=<prefix>) reads <prefix>_<run>.rou.xml (multi_signal.py:33-38,123-124).  A
batched handle does it per environment: it keeps its scenario -- net, routes, signals, capacity -- and every environment inserts the
trips of its own variant.  A variant is a Scenario that differs from the base in `trip_depart / trip_route / trip_vtype / trips_cum`
alone and has the base's number of trips; a trip that shall never enter is scheduled at horizon + 1.  Such a Scenario is also what the
CPU oracle takes (OracleEnv(variant, env_index=e)): environment e of a handle with variants equals the oracle on e's variant."""
import dataclasses

import numpy as np

MAX_DEPART = 65534      # departs travel as 16 bits on the device (0xFFFF: no trip)


def trips_cum(depart, horizon):
    """trips_cum[t] = number of trips with depart <= t, t = 0 .. horizon + 1 (as compile_scenario counts them)"""
    return np.searchsorted(np.asarray(depart), np.arange(int(horizon) + 2), side='right').astype(np.int32)


def scheduled(sc):
    """the demand of a variant: its trips with depart <= horizon (padding trips, at horizon + 1, are not demand)"""
    return int((np.asarray(sc.arrays['trip_depart']) <= sc.horizon).sum())


def common_vtype(vtype):
    """the most common vehicle type of a demand, ties to the lower index (resco_tables.h: PackedTables::common_vtype)"""
    return int(np.bincount(np.asarray(vtype, np.int64)).argmax())


def with_trips(sc, depart, route, vtype, trip_ids=None):
    """A copy of `sc` with other trips: trip_depart / trip_route / trip_vtype replaced and trips_cum recounted, everything else
    shared with `sc`.  Refuses a length other than sc.n_trips, departs that decrease, are negative or above 65534, a route
    >= n_routes, a vtype >= n_vtypes."""
    depart, route, vtype = (np.asarray(a) for a in (depart, route, vtype))
    n = sc.n_trips
    for name, a in (('depart', depart), ('route', route), ('vtype', vtype)):
        if a.ndim != 1 or len(a) != n:
            raise ValueError('with_trips: %s has shape %s, the scenario has %d trips' % (name, a.shape, n))
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError('with_trips: %s must be integers, got %s' % (name, a.dtype))
    if n and (int(depart.min()) < 0 or int(depart.max()) > MAX_DEPART):
        raise ValueError('with_trips: departs must lie in 0 .. %d' % MAX_DEPART)
    if n and bool((np.diff(depart.astype(np.int64)) < 0).any()):
        raise ValueError('with_trips: departs must be non-decreasing')
    n_vtypes = int(sc.arrays['vtype_params'].shape[0])
    if n and (int(route.min()) < 0 or int(route.max()) >= sc.n_routes):
        raise ValueError('with_trips: a route is outside 0 .. %d' % (sc.n_routes - 1))
    if n and (int(vtype.min()) < 0 or int(vtype.max()) >= n_vtypes):
        raise ValueError('with_trips: a vehicle type is outside 0 .. %d' % (n_vtypes - 1))
    if trip_ids is not None and len(trip_ids) != n:
        raise ValueError('with_trips: %d trip ids for %d trips' % (len(trip_ids), n))
    arrays = dict(sc.arrays)
    arrays['trip_depart'] = np.ascontiguousarray(depart, np.int32)
    arrays['trip_route'] = np.ascontiguousarray(route, np.int32)
    arrays['trip_vtype'] = np.ascontiguousarray(vtype, np.int32)
    arrays['trips_cum'] = trips_cum(arrays['trip_depart'], sc.horizon)
    return dataclasses.replace(sc, arrays=arrays, trip_ids=list(sc.trip_ids) if trip_ids is None else list(trip_ids))


def demand_variant(sc, seed, keep=(1.0, 1.0), jitter_s=0, resample=True):
    """One variant of sc's demand, a pure function of the arguments (numpy default_rng(seed)):
    resample   every trip is drawn from the base trips (route, vtype, depart together) with replacement;
    jitter_s   the depart is shifted by a uniform integer in [-jitter_s, jitter_s] and clipped to [0, horizon];
    keep       (lo, hi): a fraction `keep` ~ U[lo, hi] of the trips stays, the others are scheduled at horizon + 1 and never enter.
    The result is sorted stably by depart; the number of trips is sc.n_trips.  A base trip that is scheduled beyond the horizon already
    (ingolstadt21 has one at horizon + 1) stays padding: it is neither jittered nor clipped into the episode.  On a map with several
    vehicle types a resampled variant whose MOST COMMON type is not the base's is refused here with a ValueError (rs_set_demand would
    refuse it: the queue unit of the lane occupancy is a constant of the handle) -- draw it with another seed."""
    rng = np.random.default_rng(seed)
    A = sc.arrays
    n, horizon = sc.n_trips, int(sc.horizon)
    lo, hi = float(keep[0]), float(keep[1])
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError('demand_variant: keep must be 0 <= lo <= hi <= 1, got %r' % (keep,))
    src = rng.integers(0, n, n) if (resample and n) else np.arange(n)
    depart = A['trip_depart'][src].astype(np.int64)
    route, vtype = A['trip_route'][src], A['trip_vtype'][src]
    ids = [sc.trip_ids[i] for i in src] if len(sc.trip_ids) == n else None
    padding = depart > horizon
    if jitter_s:
        depart = depart + rng.integers(-int(jitter_s), int(jitter_s) + 1, n)
    depart = np.where(padding, horizon + 1, np.clip(depart, 0, horizon))
    frac = lo + (hi - lo) * float(rng.random())
    n_drop = n - int(round(frac * n))
    if n_drop > 0:
        depart[rng.permutation(n)[:n_drop]] = horizon + 1
    if n and common_vtype(vtype) != common_vtype(A['trip_vtype']):
        raise ValueError('demand_variant: seed %r gives a variant whose most common vehicle type is %d, the scenario\'s is %d: a handle '
                         'refuses it (rs_set_demand), draw another seed' % (seed, common_vtype(vtype), common_vtype(A['trip_vtype'])))
    order = np.argsort(depart, kind='stable')
    return with_trips(sc, depart[order].astype(np.int32), route[order], vtype[order], None if ids is None else [ids[i] for i in order])


def demand_set(sc, K, seed, **kw):
    """K variants: demand_variant(sc, s_k, **kw) with the seeds s_k spawned from `seed` (numpy SeedSequence: an int or a sequence of
    ints), so that the sets of different seeds do not share variants."""
    entropy = [int(x) for x in seed] if isinstance(seed, (tuple, list)) else int(seed)
    seeds = np.random.SeedSequence(entropy).generate_state(int(K), np.uint64)
    return [demand_variant(sc, int(s), **kw) for s in seeds]


TRAIN_STREAM, EVAL_STREAM = 0, 1


def episode_set(sc, K, seed, episode, **kw):
    """the set a training tool draws for an episode: a function of (seed, episode), so that a resumed run draws what the first run drew"""
    return demand_set(sc, K, (TRAIN_STREAM, int(seed), int(episode)), **kw)


def eval_set(sc, K, seed, **kw):
    """held-out variants for an evaluation: seeds no episode_set shares"""
    return demand_set(sc, K, (EVAL_STREAM, int(seed)), **kw)


def per_variant_mean(values, env_variant, K):
    """mean of a per-environment figure over the environments of every variant -> [K] (nan: a variant no environment runs)"""
    values, env_variant = np.asarray(values, np.float64), np.asarray(env_variant)
    return np.array([values[env_variant == k].mean() if (env_variant == k).any() else np.nan for k in range(int(K))])


def tool_flags(argv):
    """--demand-variants K[,jitter_s[,keep_lo,keep_hi]] and --eval-demand K[,...] (the same form; K alone: the training spec's jitter
    and keep) taken out of an argument list -> (keyword arguments for the tool's main(), the remaining arguments)"""
    kw, rest, i = {}, [], 0
    while i < len(argv):
        if argv[i] in ('--demand-variants', '--eval-demand'):
            if i + 1 >= len(argv):
                raise SystemExit('%s needs a value' % argv[i])
            parse_spec(argv[i + 1])
            kw['demand_variants' if argv[i] == '--demand-variants' else 'eval_demand'] = argv[i + 1]
            i += 2
            continue
        rest.append(argv[i])
        i += 1
    return kw, rest


def env_variants(n_envs, env_base, K):
    """the default map environment -> variant: (env_base + e) % K, keyed by the GLOBAL environment index so that the pipes or GPU
    shards of a split batch get what the single batch gets"""
    return ((int(env_base) + np.arange(int(n_envs), dtype=np.int64)) % int(K)).astype(np.int32)


def parse_spec(text):
    """'K[,jitter_s,keep_lo,keep_hi]' (the tools' --demand-variants) -> (K, dict(jitter_s=, keep=)); None / '' / '0' -> (0, {})"""
    if not text:
        return 0, {}
    parts = str(text).split(',')
    if len(parts) not in (1, 2, 4):
        raise ValueError('demand variants: K[,jitter_s[,keep_lo,keep_hi]], got %r' % (text,))
    K = int(parts[0])
    if K < 0:
        raise ValueError('demand variants: K must be >= 0')
    kw = {}
    if len(parts) >= 2:
        kw['jitter_s'] = int(parts[1])
    if len(parts) == 4:
        kw['keep'] = (float(parts[2]), float(parts[3]))
    return K, kw
