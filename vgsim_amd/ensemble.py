"""Replicate ensembles: many independent seeded trajectories of one model on one GPU, one GPU per process.

The reference has no notion of an ensemble (users start separate ``Simulator`` processes by hand, SURVEY.md
§8e); this is the data-parallel axis the engine shards: replicate r of rank k runs on GPU k as its own
persistent wavefront, nothing is exchanged while simulating, and the only collective is one gather of the
fixed-shape summary trajectories ``[replicates, points, populations, 2]`` to rank 0 (RCCL over xGMI when the
process group uses the ``nccl`` backend, gloo on CPU in the tests).
"""
import ctypes as C

import numpy as np

from . import _capi


class EnsembleResult:
    """Per-replicate outcome of one ensemble call (numpy arrays of length n_replicates)."""

    def __init__(self, R):
        z = lambda: np.zeros(R, dtype=np.int64)  # noqa: E731
        self.events = z()           # events.ptr
        self.loop_iterations = z()  # incl. rejected migrations
        self.restarts = z()
        self.kernel_ms = 0.0

    @property
    def total_events(self):
        return int(self.events.sum())


def _check_scenarios(base, scenarios, scenario_of, R):
    """The checks of a scenario ensemble, before any engine exists: (models, scenario_of as an int32 array).  Everything a scenario
    does not own — dimensions, population sizes (the start state is shared), recombination settings — must equal the base's."""
    models = [getattr(s, "simulation", s) for s in scenarios]
    if not models:
        raise ValueError("scenarios must hold at least one model")
    G = len(models)
    for g, m in enumerate([base] + models):
        who = "the base simulator" if g == 0 else "scenario %d" % (g - 1)
        if m._memory_optimization:
            raise ValueError("%s: scenario ensembles do not take memory_optimization=True" % who)
        if g == 0:
            continue
        if (m.sites, m.popNum, m.susNum) != (base.sites, base.popNum, base.susNum):
            raise ValueError("%s: its dimensions (sites, populations, susceptibility groups) = %r differ from the base simulator's %r"
                             % (who, (m.sites, m.popNum, m.susNum), (base.sites, base.popNum, base.susNum)))
        if not np.array_equal(m.sizes, base.sizes):
            raise ValueError("%s: its population sizes differ from the base simulator's (every scenario runs from the one start state)" % who)
        if m.recombination != base.recombination or m.genome_length != base.genome_length or \
                not np.array_equal(m.sitesPosition, base.sitesPosition):
            raise ValueError("%s: its recombination probability, genome length or site positions differ from the base simulator's "
                             "(recombination settings are shared by all scenarios)" % who)
        m._check_supported()
    of = np.arange(R, dtype=np.int64) % G if scenario_of is None else np.asarray(scenario_of)
    if of.shape != (R,):
        raise ValueError("scenario_of must hold one scenario index per replicate: got shape %r for %d replicates" % (of.shape, R))
    if not np.issubdtype(of.dtype, np.integer) or (R and (of.min() < 0 or of.max() >= G)):
        raise ValueError("scenario_of must hold integers in [0, %d)" % G)
    return models, np.ascontiguousarray(of, dtype=np.int32)


SUMMARY_METHODS = ('linear', 'lower', 'higher')


def _summary_position(q, m):
    """Where quantile ``q`` lies among ``m`` sorted values, as a fractional index q (m - 1) in [0, m - 1].  Evaluated in numpy's
    order for its default method (``m q + (1 - q) - 1``), so that the fractional part is numpy's to the last bit."""
    q = np.asarray(q, dtype=np.float64)
    return np.clip(m * q + (1.0 + q * -1.0) - 1.0, 0.0, float(m - 1))


def _summary_ranks(q, m, method):
    """The ranks (0-based indices into a group's ``m`` values sorted ascending) the device is asked for, per quantile ``q``:
    'lower': floor(q (m - 1)); 'higher': its ceiling; 'linear': both neighbours of the fractional index, the Q lower ones, then
    the Q upper ones (``min(lower + 1, m - 1)``).  int64; all zeros for an empty group."""
    q = np.asarray(q, dtype=np.float64).ravel()
    if method not in SUMMARY_METHODS:
        raise ValueError("method must be 'linear', 'lower' or 'higher'")
    if m <= 0:
        return np.zeros(len(q) * (2 if method == 'linear' else 1), dtype=np.int64)
    if method == 'linear':
        lo = np.floor(_summary_position(q, m)).astype(np.int64)
        return np.concatenate([lo, np.minimum(lo + 1, m - 1)])
    pos = (m - 1) * q
    return (np.floor(pos) if method == 'lower' else np.ceil(pos)).astype(np.int64)


def _summary_lerp(lower, upper, q, m):
    """The 'linear' quantile from the values at the two ranks ``_summary_ranks(q, m, 'linear')`` asks for (``q`` broadcasts
    against them): with t the fractional part of the index q (m - 1), ``lower + (upper - lower) t``, taken from the upper end
    (``upper - (upper - lower)(1 - t)``) when t >= 0.5 — numpy's rule."""
    pos = _summary_position(q, m)
    t = pos - np.floor(pos)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    d = upper - lower
    return np.where(t >= 0.5, upper - d * (1.0 - t), lower + d * t)


def _summary_groups(by, replicates, R, scenario_of, n_scenarios):
    """(group_of [R] int64 with -1 for replicates left out, G) of a ``trajectory_summary`` call; ValueError for bad arguments."""
    if isinstance(by, str):
        if by != 'auto':
            raise ValueError("by must be 'auto' or an integer array of one group label per replicate")
        group_of = np.zeros(R, dtype=np.int64) if scenario_of is None else np.asarray(scenario_of, dtype=np.int64).copy()
        G = 1 if scenario_of is None else int(n_scenarios)
    else:
        lab = np.asarray(by)
        if lab.shape != (R,) or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError("by must hold one integer group label per replicate: got shape %r, dtype %s for %d replicates"
                             % (lab.shape, lab.dtype, R))
        if R and lab.min() < 0:
            raise ValueError("group labels must not be negative")
        if R and lab.max() >= R:   # (R replicates fill at most R groups: a stray large label would only size the outputs)
            raise ValueError("group labels must be below the number of replicates (%d): got %d" % (R, lab.max()))
        group_of = lab.astype(np.int64)
        G = int(group_of.max()) + 1 if R else 1
    if replicates is not None:
        reps = np.asarray(replicates)
        if reps.dtype == bool and reps.shape == (R,):
            reps = np.nonzero(reps)[0]
        reps = reps.astype(np.int64).ravel()
        if len(reps) and (reps.min() < 0 or reps.max() >= R):
            raise ValueError("replicate index out of range")
        keep = np.zeros(R, dtype=bool)
        keep[reps] = True
        group_of[~keep] = -1
    return np.ascontiguousarray(group_of), G


class TrajectorySummary:
    """What ``Ensemble.trajectory_summary`` returns: per group of replicates, across its members, for every time point,
    population and compartment (0 = infectious, 1 = susceptible).

    ``groups`` [G] the group labels (scenario indices for ``by='auto'`` on a scenario ensemble); ``count`` [G] members;
    ``sum`` [G, T, P, 2] int64 and ``sumsq`` [G, T, P, 2] Python integers (object array, put together on first use from
    ``sumsq_words`` [G, T, P, 2, 2] uint64: low, high), both exact; ``mean`` [G, T, P, 2]
    = sum / count; ``min``, ``max`` [G, T, P, 2] int64; ``q`` the quantiles asked for and ``quantiles`` [G, Q, T, P, 2]
    float64 (``method``); ``var(ddof=0)``.  An empty group has count 0, zero sum, min and max, and NaN mean, variance
    and quantiles.  ``kernel_ms``, ``copy_ms``, ``wall_ms``: device time of the kernels, uploads and read-out, the whole library call;
    ``passes``: chunks of columns."""

    _sumsq = None

    @property
    def sumsq(self):
        if self._sumsq is None:
            w = self.sumsq_words
            self._sumsq = w[..., 0].astype(object) + w[..., 1].astype(object) * (1 << 64)
        return self._sumsq

    @sumsq.setter
    def sumsq(self, value):
        self._sumsq = value

    def var(self, ddof=0):
        """Variance across the group's members from the exact integers, ``(n sumsq - sum^2) / (n (n - ddof))`` with the numerator formed
        in integer arithmetic and one rounding in the division: population variance by default; NaN where n <= ddof."""
        out = np.full(self.sum.shape, np.nan)
        for g, n in enumerate(self.count):
            n = int(n)
            if n > ddof:
                s = self.sum[g].astype(object)
                out[g] = ((n * self.sumsq[g] - s * s) / (n * (n - ddof))).astype(np.float64)
        return out


def _summary_request(group_of, G, q, method, cols):
    """A ``VgxTrajSummaryIO`` with its outputs allocated for the column summary of a matrix whose columns have the shape ``cols``
    (rows labelled by ``group_of`` in [-1, G)): (io, finish), where ``finish()`` builds the :class:`TrajectorySummary` once the
    library has filled the outputs."""
    count = np.bincount(group_of[group_of >= 0], minlength=G)
    ranks = np.ascontiguousarray(np.stack([_summary_ranks(q, int(m), method) for m in count]))
    K, N = ranks.shape[1], int(np.prod(cols))
    io = _capi.VgxTrajSummaryIO()
    out = {k: np.zeros((G, N), dtype=np.int64) for k in ("sum", "min", "max")}
    out["count"] = np.zeros(G, dtype=np.int64)
    out["stat"] = np.zeros((G, max(K, 1), N), dtype=np.int64)
    sumsq = np.zeros((G, N, 2), dtype=np.uint64)
    io.G, io.group_of, io.K, io.ranks = G, _capi._p(group_of), K, _capi._p(ranks)
    for k, a in out.items():
        setattr(io, k, _capi._p(a))
    io.sumsq = sumsq.ctypes.data_as(C.POINTER(C.c_uint64))
    cols = tuple(int(c) for c in cols)

    def finish(_alive=(group_of, ranks)):   # (the input arrays live as long as this closure)
        s = TrajectorySummary()
        shape = (G,) + cols
        s.groups, s.count, s.q, s.method = np.arange(G), out["count"], q, method
        s.sum, s.min, s.max = out["sum"].reshape(shape), out["min"].reshape(shape), out["max"].reshape(shape)
        s.sumsq_words = sumsq.reshape(shape + (2,))
        n = s.count.astype(np.float64).reshape((G,) + (1,) * len(cols))
        with np.errstate(invalid='ignore', divide='ignore'):
            s.mean = s.sum / n
        Q = len(q)
        stat = out["stat"][:, :K].reshape((G, K) + cols)
        if method == 'linear':
            s.quantiles = np.stack([_summary_lerp(stat[g, :Q], stat[g, Q:], q.reshape((Q,) + (1,) * len(cols)), int(m)) if m else
                                    np.full((Q,) + cols, np.nan) for g, m in enumerate(s.count)])
        else:
            s.quantiles = stat.astype(np.float64)
            s.quantiles[s.count == 0] = np.nan
        s.passes, s.kernel_ms, s.copy_ms, s.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return s
    return io, finish


def _summary_quantiles(quantiles, method):
    """The checks on ``quantiles`` and ``method`` every summary shares: the quantiles as a flat float64 array."""
    if method not in SUMMARY_METHODS:
        raise ValueError("method must be 'linear', 'lower' or 'higher'")
    q = np.asarray(quantiles, dtype=np.float64).ravel()
    if not np.all((q >= 0.0) & (q <= 1.0)):   # (NaN fails too)
        raise ValueError("quantiles must lie in [0, 1]")
    return q


class Incidence:
    """What ``Ensemble.incidence`` returns: event counts per selected replicate, time bin, population and channel.

    ``counts`` [n, T, P, 7] int32 (int64 from ``tau_incidence``; None when the call had ``counts=False``), channel k as ``CHANNELS`` names it: births, deaths
    (recoveries), samplings (recorded cases), mutations, immunity changes, migrations counted where they arrive (a new infection
    there) and where they depart from; ``edges`` [T + 1] the bin edges (bin b holds edges[b] <= t < edges[b + 1]); ``outside``
    [n, 2] the events of every replicate before ``edges[0]`` and from ``edges[T]`` on; ``replicates`` [n]; ``summary`` a
    :class:`TrajectorySummary` over the [T, P, 7] columns, or None; ``passes``, ``kernel_ms``, ``clock_ms``, ``wall_ms``."""

    CHANNELS = _capi.INCIDENCE_CHANNELS

    def new_infections(self):
        """Births plus arriving migrations, [n, T, P]."""
        return self.counts[..., 0] + self.counts[..., 5]


def _incidence_edges(edges, bins, window):
    """The bin edges of an ``incidence`` call as a float64 array; ValueError for bad arguments."""
    if (edges is None) == (bins is None):
        raise ValueError("give either edges or bins (with window), not both and not neither")
    if edges is None:
        bins = int(bins)
        if bins < 1:
            raise ValueError("bins must be at least 1")
        if window is None or len(window) != 2:
            raise ValueError("bins needs window=(t0, t1)")
        t0, t1 = float(window[0]), float(window[1])
        with np.errstate(invalid='ignore', over='ignore'):   # (a window that is not finite is refused below)
            e = t0 + (np.arange(bins + 1, dtype=np.float64) * (t1 - t0)) / bins
        e[bins] = t1
    else:
        e = np.array(edges, dtype=np.float64).ravel()
        if len(e) < 2:
            raise ValueError("edges must hold at least two values")
    if not np.all(np.isfinite(e)):
        raise ValueError("edges must be finite")
    if not np.all(e[1:] > e[:-1]):
        raise ValueError("edges must increase strictly")
    return np.ascontiguousarray(e)


class Flows:
    """What ``Ensemble.flows`` returns: new infections per selected replicate, time bin, source population, destination
    population and variant class.

    ``counts`` [n, T, P, P, V] int32 (int64 from ``tau_flows``) indexed ``[r, b, src, dst, c]`` (None when the call had ``counts=False``): a birth in p counts
    at (p, p), a migration at (population, newPopulation); ``edges`` [T + 1] the bin edges (bin b holds edges[b] <= t <
    edges[b + 1]); ``variant_of`` [H] the class of every haplotype (-1: not tracked); ``outside`` [n, 2] the events of every
    replicate before ``edges[0]`` and from ``edges[T]`` on; ``replicates`` [n]; ``summary`` a :class:`TrajectorySummary` over the
    [T, P, P, V] columns, or None; ``form`` the table the counting workgroups kept ('dense' or 'split': no value depends on it);
    ``passes``, ``kernel_ms``, ``clock_ms``, ``wall_ms``."""

    def local(self):
        """Transmissions within a population, [n, T, P, V]: the diagonal."""
        return np.ascontiguousarray(np.moveaxis(np.diagonal(self.counts, axis1=2, axis2=3), -1, 2))

    def new_infections(self):
        """New infections per destination, [n, T, dst, V]: the sum over src, the diagonal included."""
        return self.counts.sum(axis=2, dtype=np.int64)

    def imports(self):
        """New infections a population received from the others, [n, T, dst, V]: the off-diagonal sum over src."""
        return self.new_infections() - self.local()

    def exports(self):
        """New infections a population caused in the others, [n, T, src, V]: the off-diagonal sum over dst."""
        return self.counts.sum(axis=3, dtype=np.int64) - self.local()

    def imported_share(self):
        """``imports() / new_infections()``, [n, T, dst, V] float64; NaN where there are no new infections."""
        total = self.new_infections()
        out = np.full(total.shape, np.nan, dtype=np.float64)
        np.divide(self.imports(), total, out=out, where=total != 0)
        return out


class Prevalence:
    """What ``Ensemble.prevalence`` returns: infectious hosts per selected replicate, grid time, population and variant class.

    ``values`` [n, T, P, V] int32 (int64 from ``tau_prevalence``, as ``final``; None when the call had ``values=False``): the hosts of class c in population p at ``times[j]``,
    events at exactly that time applied; ``final`` [n, P, V] int32 the same after the whole chain; ``times`` [T]; ``variant_of``
    [H] the class of every haplotype (-1: not tracked); ``outside`` [n, 2] the events of every replicate up to ``times[0]`` and
    after ``times[T - 1]``; ``replicates`` [n]; ``summary`` a :class:`TrajectorySummary` over the [T, P, V] columns, or None;
    ``passes``, ``kernel_ms``, ``clock_ms``, ``wall_ms``."""

    def share(self):
        """Every class's share of the tracked infected hosts of its population, [n, T, P, V] float64: ``values`` over their sum
        across classes, 0 where no tracked host is infected."""
        total = self.values.sum(axis=-1, keepdims=True, dtype=np.int64)
        out = np.zeros(self.values.shape, dtype=np.float64)
        np.divide(self.values, total, out=out, where=total != 0)
        return out


class Lineages:
    """What ``Ensemble.lineages`` returns: the ancestral lineages of the sampled cases per selected replicate, grid time, population
    and variant class: the tree's counterpart of :class:`Prevalence`.

    ``values`` [n, T, P, V] int32 (None when the call had ``values=False``): the lineages of the sample's tree alive at
    ``times[j]`` in population p that carry a haplotype of class c, events at exactly that time applied; ``root`` [n, P, V] int32
    the same before the first event (with every haplotype tracked it sums to 1: the root of the tree); ``times`` [T];
    ``variant_of`` [H] the class of every haplotype (-1: not tracked); ``replicates`` [n]; ``status``, ``status_arg`` [n] 0 or
    why the walk of row i stopped, as :class:`GenealogyBatch` (``message(i)``; such a row holds zeros), ``ok`` = ``status == 0``;
    ``records`` [n] the lineage records of every walk; ``rng_raw`` [n, 6] the generator after the walk, that of
    ``genealogies()``; ``summary`` a :class:`TrajectorySummary` over the [T, P, V] columns, or None; ``passes`` (walk passes),
    ``kernel_ms`` (``stage_ms``: walk, binning and suffix sum apart), ``clock_ms``, ``wall_ms``.  ``Ensemble.tau_lineages`` returns
    the same class for tau replicates: ``rng_raw`` is then that of ``tau_genealogies()`` (all six words used), ``stage_ms`` has
    four entries (canonicalise, walk, binning, suffix sum) and ``clock_ms`` is the host's cuts."""

    @property
    def ok(self):
        return self.status == 0

    def message(self, i):
        """Text of row i's status: what ``Ensemble.genealogy`` raises for that replicate ('' when its walk succeeded)."""
        return _capi.genealogy_message(int(self.status[i]), int(self.status_arg[i]))

    def total(self):
        """Lineages alive at every grid time, [n, T] int64: ``values`` summed over populations and classes."""
        return self.values.sum(axis=(-1, -2), dtype=np.int64)

    def sampled_share(self, pv):
        """The share of the infectious hosts that are ancestors of the sample, [n, T, P, V] float64: ``values / pv.values`` for the
        :class:`Prevalence` ``pv`` of the same replicates, grid and variants; NaN where ``pv.values`` is not positive."""
        if pv.values is None or self.values is None or pv.values.shape != self.values.shape:
            raise ValueError("sampled_share needs the values of a prevalence() call on the same replicates, grid and variants")
        out = np.full(self.values.shape, np.nan, dtype=np.float64)
        np.divide(self.values, pv.values, out=out, where=pv.values > 0)
        return out


class TreeEvents:
    """What ``Ensemble.tree_events`` and ``Ensemble.tau_tree_events`` return: the events of every selected replicate's sampled tree
    per interval of the grid, population, variant class and kind: the tree's counterpart of :class:`Incidence` and
    :class:`Flows`, from the walk and the lineage log of :class:`Lineages`.

    ``counts`` [n, T + 1, P, V, 7] int32 (None when the call had ``values=False``): interval i = 0 .. T holds the events after
    ``times[i - 1]`` up to and including ``times[i]`` (interval 0 from the start, interval T the tail after the last grid time),
    the last axis the channels ``CHANNELS``, each with an accessor of its name that gives [n, T + 1, P, V]: ``samples`` (a tip),
    ``coalescences`` (an internal node; in the population of the lineages it joins), ``mutations_within`` (a lineage's mutation
    inside one class), ``mutations_out`` and ``mutations_in`` (between classes, at the class left and the class entered),
    ``departures`` and ``arrivals`` (a lineage moved by a migration without coalescing, at its source and its destination).
    ``net()`` is their signed sum, the net change of the lineages of a cell, and ``lineages()`` the :class:`Lineages` that
    follows from it.  ``times`` [T]; ``variant_of`` [H]; ``replicates`` [n]; ``status``, ``status_arg``, ``ok``, ``message(i)``,
    ``records``, ``rng_raw`` as :class:`Lineages` (a failed walk's row holds zeros); ``summary`` a :class:`TrajectorySummary`
    over the [T + 1, P, V, 7] columns, or None; ``passes``, ``kernel_ms`` (``stage_ms``: walk and binning apart; for tau
    replicates canonicalise, walk and binning), ``clock_ms``, ``wall_ms``."""

    CHANNELS = _capi.TREE_EVENT_CHANNELS

    @property
    def ok(self):
        return self.status == 0

    def message(self, i):
        """Text of row i's status: what ``Ensemble.genealogy`` raises for that replicate ('' when its walk succeeded)."""
        return _capi.genealogy_message(int(self.status[i]), int(self.status_arg[i]))

    def net(self):
        """The net change of the lineages per interval and cell, [n, T + 1, P, V] int64: coalescences - samples + mutations_in -
        mutations_out + arrivals - departures."""
        c = self.counts.astype(np.int64)
        return c[..., 1] - c[..., 0] + c[..., 4] - c[..., 3] + c[..., 6] - c[..., 5]

    def lineages(self):
        """The :class:`Lineages` of the same walk, computed on the host from ``counts``: no lineage is alive after the last event,
        so ``root`` is minus the net change of all intervals and ``values[:, j]`` the root plus that of the intervals 0 .. j."""
        net = self.net()
        ln = Lineages()
        root = -net.sum(axis=1)
        ln.root = root.astype(np.int32)
        ln.values = (root[:, None] + np.cumsum(net[:, :-1], axis=1)).astype(np.int32)
        ln.times, ln.variant_of, ln.replicates = self.times, self.variant_of, self.replicates
        ln.status, ln.status_arg, ln.records, ln.rng_raw = self.status, self.status_arg, self.records, self.rng_raw
        ln.summary = None
        ln.passes, ln.kernel_ms, ln.clock_ms, ln.wall_ms, ln.stage_ms = self.passes, self.kernel_ms, self.clock_ms, self.wall_ms, self.stage_ms
        return ln

    # one accessor per channel, [n, T + 1, P, V]
    def samples(self):
        return self.counts[..., 0]

    def coalescences(self):
        return self.counts[..., 1]

    def mutations_within(self):
        return self.counts[..., 2]

    def mutations_out(self):
        return self.counts[..., 3]

    def mutations_in(self):
        return self.counts[..., 4]

    def departures(self):
        return self.counts[..., 5]

    def arrivals(self):
        return self.counts[..., 6]


class TreeShapes:
    """What ``Ensemble.tree_shapes`` returns: one row of scalars per selected replicate's sampled tree: its balance, depth and
    branch statistics, the summaries simulated trees are compared by.

    ``stats`` [n, 12] int64 in the order of ``STATS`` and ``lengths`` [n, 7] float64 in the order of ``LENGTHS``, each column also
    an attribute of its name ([n]).  A tip is a node without children; ``n_v`` the tips below node v.  ``tips``; ``internal``
    (= tips - 1); ``cherries`` (nodes with two tip children); ``pitchforks`` (``n_v == 3``); ``sackin`` (sum of the tips' depths in
    edges); ``colless`` (sum over internal nodes of the difference of their two children's ``n``); ``max_depth``; ``depth_sumsq``
    (sum of the tips' squared depths); ``ladder_nodes`` (nodes with exactly one tip child); ``max_ladder`` (the longest chain of
    them); ``root_event`` and ``last_tip_event`` (the event indices of the root and of node 0, the latest sample).  With
    ``b_i`` the branch above node i in time: ``root_time``, ``last_tip_time``, ``length`` (sum of ``b_i``), ``external_length``
    (over the tips), ``length_sumsq``, ``tip_height_sum`` (sum over the tips of their time above the root), ``max_branch``.
    ``replicates`` [n]; ``status``, ``status_arg``, ``ok``, ``message(i)``, ``rng_raw`` as :class:`GenealogyBatch`: the row of a
    replicate whose walk failed holds zeros and NaN lengths, and the derived values are NaN there.  ``passes``, ``kernel_ms``
    (walk, shape), ``clock_ms`` (the host clock with the two node copies), ``wall_ms``."""

    STATS = _capi.TREE_SHAPE_STATS
    LENGTHS = _capi.TREE_SHAPE_LENGTHS

    def __getattr__(self, name):   # one attribute per column
        if name in TreeShapes.STATS:
            return self.stats[:, TreeShapes.STATS.index(name)]
        if name in TreeShapes.LENGTHS:
            return self.lengths[:, TreeShapes.LENGTHS.index(name)]
        raise AttributeError(name)

    @property
    def ok(self):
        return self.status == 0

    def message(self, i):
        """Text of row i's status: what ``Ensemble.genealogy`` raises for that replicate ('' when its walk succeeded)."""
        return _capi.genealogy_message(int(self.status[i]), int(self.status_arg[i]))

    def _ratio(self, num, den, where=None):
        out = np.full(len(self.status), np.nan, dtype=np.float64)
        ok = self.ok & (den != 0) if where is None else self.ok & where
        np.divide(num, den, out=out, where=ok)
        return out

    def height(self):
        """The tree's height in time: ``last_tip_time - root_time``."""
        return np.where(self.ok, self.last_tip_time - self.root_time, np.nan)

    def mean_depth(self):
        """Mean depth of a tip in edges: ``sackin / tips``."""
        return self._ratio(self.sackin.astype(np.float64), self.tips.astype(np.float64))

    def depth_variance(self):
        """Variance of the tips' depths: ``depth_sumsq / tips - mean_depth() ** 2``."""
        return self._ratio(self.depth_sumsq.astype(np.float64), self.tips.astype(np.float64)) - self.mean_depth() ** 2

    def colless_normalized(self):
        """``colless`` over its maximum ``(tips - 1)(tips - 2) / 2``, the caterpillar tree's; NaN at two tips."""
        t = self.tips.astype(np.float64)
        return self._ratio(self.colless.astype(np.float64), (t - 1) * (t - 2) / 2, where=self.tips > 2)

    def mean_branch(self):
        """Mean branch length: ``length / (2 tips - 2)``."""
        return self._ratio(self.length, 2.0 * self.tips - 2)

    def external_share(self):
        """The share of the tree's length on branches that end in a tip: ``external_length / length``."""
        return self._ratio(self.external_length, self.length)


class MutationSpectrum:
    """What ``Ensemble.mutation_spectrum`` returns: the mutation records of every selected replicate's sampled tree reduced to their
    clade sizes: the site-frequency spectrum in log2 bins, the substitution counts and the sums its scalar estimators are made of.

    A record sits on the branch above its node; its frequency in the sample is ``c``, the number of tips below that node.  Every
    record is one mutation event (the infinite-sites reading of a model with finitely many sites and recurrent mutation).  With
    ``sites`` = S: ``spectrum`` [n, S, 32] int64, records of site s with ``floor(log2 c) == b``; ``substitutions`` [n, S, 4, 4],
    records by site, ancestral and derived state; ``sums`` [n, S, 3] in the order of ``SUMS``: ``clade_sum`` (sum of c),
    ``clade_sumsq`` (sum of c^2), ``pair_sum`` (sum of c (tips - c)); ``stats`` [n, 4] in the order of ``STATS``, each column also an
    attribute: ``tips``, ``mutations``, ``fixed`` (records with c == tips: on the root), ``max_clade``.  All exact integers: the same
    bits on every path.  ``replicates`` [n]; ``status``, ``status_arg``, ``ok``, ``message(i)``, ``rng_raw`` as
    :class:`GenealogyBatch`: the row of a replicate whose walk failed holds zeros, and the derived values are NaN there and wherever
    a denominator is 0.  ``passes``, ``kernel_ms`` (walk, spectrum), ``wall_ms``."""

    SUMS = _capi.MUTATION_SPECTRUM_SUMS
    STATS = _capi.MUTATION_SPECTRUM_STATS
    BINS = _capi.MUTATION_SPECTRUM_BINS

    def __getattr__(self, name):   # one attribute per column of stats
        if name in MutationSpectrum.STATS:
            return self.stats[:, MutationSpectrum.STATS.index(name)]
        raise AttributeError(name)

    @property
    def ok(self):
        return self.status == 0

    def message(self, i):
        """Text of row i's status: what ``Ensemble.genealogy`` raises for that replicate ('' when its walk succeeded)."""
        return _capi.genealogy_message(int(self.status[i]), int(self.status_arg[i]))

    def _ratio(self, num, den, where=None):
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        ok = self.ok & (den != 0) if where is None else self.ok & where
        if num.ndim == 2:
            den, ok = np.broadcast_to(den[:, None], num.shape), np.broadcast_to(ok[:, None], num.shape)
        out = np.full(num.shape, np.nan, dtype=np.float64)
        np.divide(num, den, out=out, where=ok)
        return out

    def _pairs(self):   # tips (tips - 1), as float64
        t = self.tips.astype(np.float64)
        return t * (t - 1.0)

    @staticmethod
    def bin_edges():
        """The lower edges of the 32 bins, ``2 ** b``: bin b holds the clade sizes ``2 ** b <= c < 2 ** (b + 1)``."""
        return 2 ** np.arange(MutationSpectrum.BINS, dtype=np.int64)

    def per_site(self):
        """Records per site, int64 [n, S]: ``spectrum.sum(-1)``."""
        return self.spectrum.sum(axis=-1)

    def singletons(self):
        """Records below which lies one tip, int64 [n]: bin 0 over all sites."""
        return self.spectrum[:, :, 0].sum(axis=-1)

    def singleton_share(self):
        """``singletons() / mutations``; NaN without records."""
        return self._ratio(self.singletons(), self.mutations)

    def substitution_matrix(self):
        """Records by ancestral and derived state over all sites, int64 [n, 4, 4]."""
        return self.substitutions.sum(axis=1)

    def pi(self, per_site=False):
        """Nucleotide diversity, the mean number of differences of two sampled tips: ``2 pair_sum / (tips (tips - 1))``, over all
        sites [n], or per site [n, S] with ``per_site``."""
        ps = self.sums[:, :, 2] if per_site else self.sums[:, :, 2].sum(axis=-1)   # (the integer sum first: exact)
        return self._ratio(2.0 * ps.astype(np.float64), self._pairs())

    def _harmonic(self):   # a1 = sum_{i < tips} 1 / i and a2 = sum_{i < tips} 1 / i^2 per row, each summed in ascending i
        a1, a2 = np.zeros(len(self.status), dtype=np.float64), np.zeros(len(self.status), dtype=np.float64)
        for k, t in enumerate(self.tips):
            i = np.arange(1, max(int(t), 1), dtype=np.float64)
            a1[k], a2[k] = np.cumsum(1.0 / i)[-1] if len(i) else 0.0, np.cumsum(1.0 / (i * i))[-1] if len(i) else 0.0
        return a1, a2

    def watterson(self):
        """Watterson's theta: ``mutations / a1`` with ``a1 = sum_{i=1}^{tips-1} 1 / i``."""
        return self._ratio(self.mutations, self._harmonic()[0])

    def theta_h(self):
        """Fay and Wu's theta_H: ``2 clade_sumsq / (tips (tips - 1))``."""
        return self._ratio(2.0 * self.sums[:, :, 1].sum(axis=-1).astype(np.float64), self._pairs())

    def fay_wu_h(self):
        """Fay and Wu's H: ``pi() - theta_h()``."""
        return self.pi() - self.theta_h()

    def tajimas_d(self):
        """Tajima's D: ``(pi - S / a1) / sqrt(e1 S + e2 S (S - 1))`` with S = ``mutations``, n = ``tips`` and
        ``a1 = sum_{i<n} 1/i``, ``a2 = sum_{i<n} 1/i^2``, ``b1 = (n + 1) / (3 (n - 1))``, ``b2 = 2 (n^2 + n + 3) / (9 n (n - 1))``,
        ``c1 = b1 - 1 / a1``, ``c2 = b2 - (n + 2) / (a1 n) + a2 / a1^2``, ``e1 = c1 / a1``, ``e2 = c2 / (a1^2 + a2)``.
        NaN without records, below two tips and where the variance term is not positive."""
        n, S = self.tips.astype(np.float64), self.mutations.astype(np.float64)
        a1, a2 = self._harmonic()
        with np.errstate(divide='ignore', invalid='ignore'):
            b1 = (n + 1.0) / (3.0 * (n - 1.0))
            b2 = 2.0 * (n * n + n + 3.0) / (9.0 * n * (n - 1.0))
            c1 = b1 - 1.0 / a1
            c2 = b2 - (n + 2.0) / (a1 * n) + a2 / (a1 * a1)
            e1 = c1 / a1
            e2 = c2 / (a1 * a1 + a2)
            var = e1 * S + e2 * S * (S - 1.0)
            good = np.isfinite(var) & (var > 0)
            d = self.pi() - self.watterson()
            return self._ratio(d, np.sqrt(np.where(good, var, 1.0)), where=good & np.isfinite(d))


class Introductions:
    """What ``Ensemble.introductions`` returns: the population labels of every selected replicate's sampled tree reduced to its
    transmission lineages: how many introductions every population received, from where, and how large the lineage is that each
    one seeded.

    The branch above a node crosses when the node's population differs from its parent's: it is then one NET introduction from
    the parent's population (src) into the node's (dst).  Moves along a branch that left no node are invisible: a lineage that went
    0 -> 2 -> 1 between two nodes counts as 0 -> 1, one that went 0 -> 1 -> 0 does not count.  The root and every node below a
    crossing branch head a transmission lineage; its size (``local``) is the number of tips reached from it without passing another
    crossing branch, possibly 0; every tip lies in exactly one lineage.  With ``pops`` = P: ``tips_by_pop`` [n, P] int64;
    ``imports`` [n, P, P] indexed ``[r, src, dst]``; ``into`` [n, P, 6] per destination over its introductions in the order of
    ``INTO``: ``count``, ``clade_sum`` (all tips below), ``local_sum``, ``local_sumsq``, ``empty`` (size 0), ``max_local``;
    ``spectrum`` [n, P, 32], introductions into dst with ``floor(log2 local) == b`` (the empty ones are in ``into`` alone);
    ``stats`` [n, 8] in the order of ``STATS``, each column also an attribute: ``tips``, ``introductions``, ``root_pop``,
    ``root_local``, ``max_local`` (the root's lineage included), ``max_clade``, ``empty``, ``pops_with_tips``.  All exact integers:
    the same bits on every path.  ``replicates`` [n]; ``status``, ``status_arg``, ``ok``, ``message(i)``, ``rng_raw`` as
    :class:`GenealogyBatch`: the row of a replicate whose walk failed holds zeros, and the ratios are NaN there and wherever a
    denominator is 0.  ``passes``, ``kernel_ms`` (walk, lineages), ``wall_ms``."""

    INTO = _capi.INTRODUCTIONS_INTO
    STATS = _capi.INTRODUCTIONS_STATS
    BINS = _capi.INTRODUCTIONS_BINS

    def __getattr__(self, name):   # one attribute per column of stats
        if name in Introductions.STATS:
            return self.stats[:, Introductions.STATS.index(name)]
        raise AttributeError(name)

    @property
    def ok(self):
        return self.status == 0

    def message(self, i):
        """Text of row i's status: what ``Ensemble.genealogy`` raises for that replicate ('' when its walk succeeded)."""
        return _capi.genealogy_message(int(self.status[i]), int(self.status_arg[i]))

    def _ratio(self, num, den):   # [n, P] / [n, P]: one float64 division per cell
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        ok = np.broadcast_to(self.ok[:, None], num.shape) & (den != 0)
        out = np.full(num.shape, np.nan, dtype=np.float64)
        np.divide(num, den, out=out, where=ok)
        return out

    @staticmethod
    def bin_edges():
        """The lower edges of the 32 bins, ``2 ** b``: bin b holds the lineage sizes ``2 ** b <= local < 2 ** (b + 1)``."""
        return 2 ** np.arange(Introductions.BINS, dtype=np.int64)

    def imports_into(self):
        """Introductions every population received, int64 [n, P]: ``imports`` summed over src (= ``into[:, :, 0]``)."""
        return self.imports.sum(axis=1)

    def exports_from(self):
        """Introductions every population seeded elsewhere, int64 [n, P]: ``imports`` summed over dst."""
        return self.imports.sum(axis=2)

    def net_flow(self):
        """``imports_into() - exports_from()``, int64 [n, P]."""
        return self.imports_into() - self.exports_from()

    def lineages(self):
        """Transmission lineages per population, int64 [n, P]: its introductions and, in the root's population, the root's
        lineage; zeros for a replicate that is not ok."""
        out = self.into[:, :, 0].copy()
        rows = np.nonzero(self.ok)[0]
        out[rows, self.root_pop[rows]] += 1
        return out

    def mean_lineage_size(self):
        """``local_sum / count`` per destination, [n, P]: the mean size of the lineages its introductions seeded."""
        return self._ratio(self.into[:, :, 2], self.into[:, :, 0])

    def size_weighted_mean(self):
        """``local_sumsq / local_sum`` per destination, [n, P]: the size of the introduced lineage a random introduced tip lies in."""
        return self._ratio(self.into[:, :, 3], self.into[:, :, 2])

    def singleton_share(self):
        """``spectrum[:, :, 0] / count`` per destination, [n, P]: introductions that seeded one sampled tip."""
        return self._ratio(self.spectrum[:, :, 0], self.into[:, :, 0])

    def empty_share(self):
        """``empty / count`` per destination, [n, P]: introductions all of whose tips lie behind further crossings."""
        return self._ratio(self.into[:, :, 4], self.into[:, :, 0])

    def observed_share(self, flows):
        """Tree introductions over the true cross-population infections per destination, [n, P]: ``imports_into()`` over
        ``flows.imports()`` (a :class:`Flows` of the same replicates in the same order) summed over its bins and variant classes,
        so the classes should cover every haplotype and the bins the whole run for the ratio to mean the sampled share."""
        if not np.array_equal(np.asarray(flows.replicates), np.asarray(self.replicates)):
            raise ValueError("observed_share() needs the Flows of the same replicates in the same order")
        return self._ratio(self.imports_into(), flows.imports().sum(axis=(1, 3), dtype=np.int64))


class Susceptibles:
    """What ``Ensemble.susceptibles`` returns: susceptible hosts per selected replicate, grid time, population and class of
    susceptibility groups.

    ``values`` [n, T, P, G] int32 (int64 from ``tau_susceptibles``, as ``final``; None when the call had ``values=False``): the
    susceptible hosts of class c in population p at ``times[j]``, events at exactly that time applied; ``final`` [n, P, G] the same
    after the whole chain; ``times`` [T]; ``class_of`` [susNum] the class of every susceptibility group (-1: not tracked);
    ``outside`` [n, 2] the events of every replicate up to ``times[0]`` and after ``times[T - 1]``; ``replicates`` [n];
    ``summary`` a :class:`TrajectorySummary` over the [T, P, G] columns, or None; ``passes``, ``kernel_ms``, ``clock_ms``,
    ``wall_ms``."""

    @classmethod
    def _of(cls, values, final, times, class_of, outside, replicates, done, io):
        sv = cls()
        sv.values, sv.final, sv.times, sv.class_of, sv.outside, sv.replicates = values, final, times, class_of, outside, replicates
        sv.summary = done() if done is not None else None
        sv.passes, sv.kernel_ms, sv.clock_ms, sv.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return sv

    def share(self):
        """Every class's share of the tracked susceptible hosts of its population, [n, T, P, G] float64: ``values`` over their sum
        across classes, 0 where no tracked host is susceptible."""
        total = self.values.sum(axis=-1, keepdims=True, dtype=np.int64)
        out = np.zeros(self.values.shape, dtype=np.float64)
        np.divide(self.values, total, out=out, where=total != 0)
        return out


class Milestones:
    """What ``Ensemble.milestones`` returns: peaks, first passages and extinctions per selected replicate, key and variant class,
    exact over every event of the chain.  The key axis holds the populations 0 .. P-1 and, at index P (or -1), all populations
    together.  Event indices count the chain's events from 0; -1 is the chain's start.

    ``peak``, ``peak_event``, ``peak_time`` [n, P+1, V]: the largest value, the first event that attains it and its time;
    ``final`` [n, P+1, V] the value after the whole chain; ``last_positive_event`` [n, P+1, V] the last event after which the cell
    holds a host (-2: never); ``first_event``, ``first_time``, ``reached`` [n, K, P+1, V]: the first event at or above
    ``thresholds[k]`` (``NEVER`` and NaN where none is, ``reached`` False); ``thresholds`` [K] int32; ``variant_of`` [H];
    ``replicates`` [n]; ``passes``, ``kernel_ms``, ``clock_ms``, ``wall_ms``.  Integer arrays are int32, times float64.

    ``Ensemble.tau_milestones`` returns the same object for tau replicates: an event is a direct event of the model's earlier
    history or one whole tau step, values are taken after all rows of a step, and ``final``, ``peak`` and ``thresholds`` are
    int64 (``clock_ms`` is the host's time for the tile and row tables)."""

    NEVER = _capi.MS_NEVER

    @property
    def extinct(self):
        """[n, P+1, V] bool: the cell held a host at some event and holds none at the end (a chain that stops at its iteration
        cap with hosts left is not extinct)."""
        return (self.last_positive_event >= -1) & (self.final == 0)

    @property
    def never_present(self):
        """[n, P+1, V] bool: the cell never held a host, the start included."""
        return self.last_positive_event == -2

    @property
    def extinction_event(self):
        """[n, P+1, V] int32: the event that emptied the cell for good, ``last_positive_event + 1``; meaningful where ``extinct``."""
        return self.last_positive_event + np.int32(1)

    def extinction_probability(self, by='auto'):
        """The share of the selected replicates of every group in which the cell is extinct, [G, P+1, V] float64 (NaN for a group
        without selected replicates).  ``by`` as ``trajectory_summary`` takes it: 'auto' is one group per scenario of a scenario
        ensemble, one group otherwise; or one integer label per replicate of the ensemble."""
        group_of, G = _summary_groups(by, None, self._R, self._scenario_of, self._n_scenarios)
        g = group_of[self.replicates]
        ext = self.extinct
        out = np.full((G,) + ext.shape[1:], np.nan)
        for k in range(G):
            if (g == k).any():
                out[k] = ext[g == k].mean(axis=0)
        return out


def _prevalence_grid(times, points, window):
    """The grid of a ``prevalence`` call as a float64 array; ValueError for bad arguments."""
    if (times is None) == (points is None):
        raise ValueError("give either times or points (with window), not both and not neither")
    if times is None:
        points = int(points)
        if points < 1:
            raise ValueError("points must be at least 1")
        if window is None or len(window) != 2:
            raise ValueError("points needs window=(t0, t1)")
        t0, t1 = float(window[0]), float(window[1])
        with np.errstate(invalid='ignore', over='ignore'):   # (a window that is not finite is refused below)
            # the trajectories' grid (t0 + j dt with dt formed once), so that both read the same instants
            g = t0 + np.arange(points, dtype=np.float64) * ((t1 - t0) / (points - 1)) if points > 1 else np.array([t0])
    else:
        g = np.array(times, dtype=np.float64).ravel()
        if len(g) < 1:
            raise ValueError("times must hold at least one value")
    if len(g) >= 1 << 24:
        raise ValueError("T = %d must be at least 1 and below 2^24" % len(g))
    if not np.all(np.isfinite(g)):
        raise ValueError("grid must be finite")
    if not np.all(g[1:] > g[:-1]):
        raise ValueError("grid must increase strictly")
    return np.ascontiguousarray(g)


class Ensemble:
    def __init__(self, simulator, n_replicates, seeds=None, device=0, scenarios=None, scenario_of=None):
        """``simulator``: a configured ``vgsim_amd.Simulator`` (or its ``.simulation`` model) giving parameters
        and the common start state; ``seeds``: one user seed per replicate (default seed, seed+1, ...).

        ``scenarios``: a sequence of configured ``Simulator`` s (or models), the COMPLETE list of parameter sets of a scenario
        ensemble; ``simulator`` then gives the start state, the dimensions and the recombination settings only.  Replicate r runs
        under ``scenarios[scenario_of[r]]`` (default ``arange(R) % len(scenarios)``) and is, bit for bit, the run of a single
        ``Simulator`` with that scenario's parameters, this start state and seed ``seeds[r]``; one launch runs all of them.
        Limits: the exact direct path on the one-replicate-per-wavefront kernel (``mode='exact'``, ``kernel`` 'auto' or 'wave');
        ``simulate_tau(..., per_scenario=True)`` on the on-device step loop (models of up to 8192 compartments); population sizes and recombination
        settings equal in all scenarios.  The contact densities a replicate starts with are its own scenario's
        (``set_contact_density``, ``set_npi``) for the lockdown state of the start state; a scenario whose model holds another
        value is refused by ``simulate`` and ``simulate_tau``."""
        self.model = getattr(simulator, "simulation", simulator)
        m = self.model
        self.R = int(n_replicates)
        self.scenarios, self.scenario_of = None, None
        if scenarios is not None:
            self.scenarios, self.scenario_of = _check_scenarios(m, scenarios, scenario_of, self.R)
        elif scenario_of is not None:
            raise ValueError("scenario_of needs scenarios")
        m._check_supported()
        self.engine = _capi.HipEngine(m.sites, m.hapNum, m.popNum, m.susNum, n_replicates=self.R, device=device)
        self.seeds = np.arange(m.user_seed, m.user_seed + self.R, dtype=np.int64) if seeds is None \
            else np.ascontiguousarray(seeds, dtype=np.int64)
        assert self.seeds.shape == (self.R,)
        self.traj_shape = None
        self._last_call = None   # ('direct' | 'tau', record_events) of the last simulate call
        self._tau_prefix = None  # events, multievent rows and lockdown records of the model when the last recorded tau call started

    def close(self):
        self.engine.close()

    def _check_scenario_contact_densities(self):
        """Every replicate of a scenario ensemble starts with its own scenario's contact densities for the lockdown state of the
        start state (the engine takes them from the set's parameters): a scenario whose model holds anything else would not be
        what runs, and is refused."""
        m = self.model
        for g, s in enumerate(self.scenarios):
            cd = np.where(np.asarray(m.lockdownON) != 0, s.contactDensityAfterLockdown, s.contactDensityBeforeLockdown)
            bad = np.nonzero(np.asarray(s.contactDensity, dtype=np.float64) != cd)[0]
            if len(bad):
                raise ValueError("scenario %d: the contact density of population %d is %r, its own settings give %r for the lockdown "
                                 "state of the start state" % (g, bad[0], float(s.contactDensity[bad[0]]), float(cd[bad[0]])))

    def _set_parameters(self):
        """The parameters of the next simulate call into the engine: the model's, or (after the check above) every scenario's."""
        if self.scenarios is None:
            self.engine.set_params(self.model)
            return
        self._check_scenario_contact_densities()
        self.engine.set_param_sets(self.scenarios, self.scenario_of)

    def _scenario_groups(self):
        """(scenario_of, number of scenarios) as the summaries' ``by='auto'`` takes them: (None, 1) without scenarios."""
        return self.scenario_of, (len(self.scenarios) if self.scenarios is not None else 1)

    def simulate(self, iterations, sample_size=None, epidemic_time=-1, attempts=200, record_events=False,
                 traj_points=0, traj_window=(0.0, 1.0), seeds=None, mode='exact', kernel='auto'):
        """Direct Gillespie for every replicate from the model's current state (``SimulatePopulation`` semantics
        per replicate, pyx:396-429).  ``mode``: 'exact' (reference summation order, bit-exact) or 'fast'
        (order-free sums).  Returns an :class:`EnsembleResult`."""
        if mode not in ('exact', 'fast', 'fast_philox'):
            raise ValueError("mode must be 'exact', 'fast' or 'fast_philox'")
        if self.scenarios is not None:
            if mode != 'exact':
                raise ValueError("a scenario ensemble runs in mode='exact' only")
            if kernel not in ('auto', 'wave'):
                raise ValueError("a scenario ensemble runs on the one-replicate-per-wavefront kernel only: kernel must be 'auto' or 'wave'")
        m, eng = self.model, self.engine
        if seeds is not None:
            self.seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        if sample_size is None:
            sample_size = iterations
        if epidemic_time is None:
            epidemic_time = -1
        # Events.CreateEvents bookkeeping on a scratch copy of the counters (the host model keeps its own log)
        ptr, size = m.events.ptr, m.events.size
        size = size + iterations if ptr == 0 else max(size, ptr + iterations)
        self._set_parameters()
        saved = (m.events.ptr, m.events.size)
        m.events.size = size
        try:
            eng.set_state(m)
        finally:
            m.events.ptr, m.events.size = saved
        eng.set_seeds(self.seeds)
        o = _capi.VgxRunOpts()
        o.record_events = 1 if record_events else 0
        o.traj_points = int(traj_points)
        o.traj_t0, o.traj_t1 = float(traj_window[0]), float(traj_window[1])
        o.mode = {'exact': 0, 'fast': 1, 'fast_philox': 2}[mode]
        o.kernel = {'auto': 0, 'wave': 1, 'lane': 2, 'quad': 3, 'quadg': 4, 'solo': 5, 'lone': 6}[kernel]
        rc = eng.lib.vgx_simulate_direct(eng.handle, int(iterations), int(sample_size), float(np.float32(epidemic_time)),
                                         int(attempts), C.byref(o))
        self._last_call = None
        eng._check(rc)
        self._last_call = ('direct', bool(record_events))
        res = EnsembleResult(self.R)
        call = eng.counters_all()
        res.events[:], res.loop_iterations[:], res.restarts[:] = call[:, 0], call[:, 1], call[:, 2]
        res.kernel_ms = eng.last_kernel_ms
        self.traj_shape = (self.R, int(traj_points), m.popNum, 2) if traj_points > 0 else None
        return res

    def simulate_tau(self, iterations, sample_size=None, epidemic_time=-1, attempts=200, record_events=False, seeds=None,
                     traj_points=0, traj_window=(0.0, 1.0), per_scenario=False):
        """Poisson tau-leaping for every replicate from the model's current state (``SimulatePopulation_tau``
        semantics per replicate, pyx:2293-2346).  ``EnsembleResult.events`` counts MULTITYPE records (steps);
        ``events_drawn`` the sum of the drawn channel multiplicities.  ``traj_points`` / ``traj_window``: summary
        trajectories as ``simulate`` bins them (a grid point gets the totals before the step that takes the time past it),
        with or without the event log; read with ``trajectories()`` / ``gather_trajectories()``.

        ``per_scenario=True`` (scenario ensembles; without it they refuse the call, as they did before they could run it):
        replicate r runs under ``scenarios[scenario_of[r]]`` and is, bit for bit, replicate k of a one-set ``Ensemble`` built on
        that scenario (holding this start state) whose seed k is ``seeds[r]``: one launch of the on-device step loop runs all
        scenarios.  The library refuses the call where that loop does not run (more than 8192 compartments,
        ``VGX_TAU_STEP_KERNELS=1``)."""
        if self.scenarios is not None and not per_scenario:
            raise ValueError("simulate_tau on a scenario ensemble runs when it is asked to: pass per_scenario=True (every replicate "
                             "under its own scenario, one launch of the on-device step loop)")
        if per_scenario and self.scenarios is None:
            raise ValueError("per_scenario=True needs a scenario ensemble (Ensemble(..., scenarios=[...]))")
        m, eng = self.model, self.engine
        if seeds is not None:
            self.seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        if sample_size is None:
            sample_size = iterations
        if epidemic_time is None:
            epidemic_time = -1
        ptr, size = m.events.ptr, m.events.size
        for _ in range(2):  # CreateEvents is called twice on the tau path (pyx:2298 -> pyx:434, pyx:2306)
            size = size + iterations if ptr == 0 else max(size, ptr + iterations)
        self._set_parameters()
        saved = (m.events.ptr, m.events.size)
        m.events.size = size
        try:
            eng.set_state(m)
        finally:
            m.events.ptr, m.events.size = saved
        eng.set_seeds(self.seeds)
        self._tau_prefix = None
        if record_events:   # the model's chain as it is now: what tau_timelines() replays in front of every replicate's steps
            ev, mv = m.events, m.multievents
            self._tau_prefix = ([ev.times[:ev.ptr].copy()] + [getattr(ev, c)[:ev.ptr].copy() for c in ev.COLUMNS],
                                [getattr(mv, c)[:mv.ptr].copy() for c in mv.COLUMNS],
                                [np.asarray(m.loc.states, dtype=np.int64), np.asarray(m.loc.populationsId, dtype=np.int64),
                                 np.asarray(m.loc.times, dtype=np.float64)])
            self._tau_prefix_mev_times = mv.times[:mv.ptr].copy()   # (tau_genealogies: nodes of a prefix row carry the row's time)
        o = _capi.VgxRunOpts()
        o.record_events = 1 if record_events else 0
        o.traj_points = int(traj_points)
        o.traj_t0, o.traj_t1 = float(traj_window[0]), float(traj_window[1])
        if self.scenarios is not None and len(self.scenarios) > 1:
            o.reserved[0] = 2     # the installed sets are meant: one per replicate
        rc = eng.lib.vgx_simulate_tau(eng.handle, int(iterations), int(sample_size), float(np.float32(epidemic_time)),
                                      int(attempts), C.byref(o))
        self._last_call = None
        eng._check(rc)
        self._last_call = ('tau', bool(record_events))
        res = EnsembleResult(self.R)
        call = eng.counters_all()
        res.events[:], res.loop_iterations[:], res.restarts[:] = call[:, 0], call[:, 1], call[:, 2]
        res.events_drawn = call[:, 3].copy()
        res.kernel_ms = eng.last_kernel_ms
        self.traj_shape = (self.R, int(traj_points), m.popNum, 2) if traj_points > 0 else None
        return res

    def replicate_state(self, replicate):
        """A host model object holding the state (compartments, counters, times) of one replicate; in a scenario ensemble a
        copy of the replicate's own scenario's model."""
        import copy
        m = copy.copy(self.model if self.scenarios is None else self.scenarios[int(self.scenario_of[replicate])])
        for name in ("susceptible", "infectious", "initial_susceptible", "initial_infectious", "totalSusceptible",
                     "totalInfectious", "lockdownON", "contactDensity"):
            setattr(m, name, getattr(self.model, name).copy())
        self.engine.get_state(m, replicate)
        return m

    def replicate_multievents(self):
        """The multievent rows of every replicate of the last ``simulate_tau(record_events=True)`` call in one read-out:
        ``(offsets, rows)`` of ``HipEngine.multievents_all`` (rows offsets[r]:offsets[r + 1] are replicate r's)."""
        if self._last_call != ('tau', True):
            raise ValueError("replicate_multievents() needs a simulate_tau(record_events=True) call first")
        return self.engine.multievents_all()

    def replicate_states_tau(self):
        """infectious, susceptible, counters and currentTime of every replicate after the last ``simulate_tau`` call in one read-out
        (``HipEngine.tau_states_all``)."""
        if self._last_call is None or self._last_call[0] != 'tau':
            raise ValueError("replicate_states_tau() needs a simulate_tau call first")
        return self.engine.tau_states_all()

    def replicate_events(self, replicate):
        """(6, n) float64 event chain of one replicate (needs ``record_events=True``)."""
        from ._model import Events
        c = self.engine.counters(replicate)
        ev = Events()
        ev.CreateEvents(max(int(c.ev_ptr), 1))
        self.engine.fetch_events(ev, replicate, c.ev_first_new, c.ev_ptr - c.ev_first_new)
        ev.ptr = c.ev_ptr
        return ev.as_array()[:, :c.ev_ptr]

    def genealogy(self, replicate, seed):
        """Backward pass (``GetGenealogy``, pyx:743-1000) over the recorded chain of one replicate of the last direct
        ``simulate(record_events=True)`` call; returns the dict of ``_capi.get_genealogy`` (tree, times, mut_*, mig_*)."""
        from ._model import Events
        m = self.replicate_state(replicate)
        chain = self.replicate_events(replicate)
        ev = Events()
        ev.CreateEvents(max(chain.shape[1], 1))
        ev.times[:chain.shape[1]] = chain[0]
        for k, name in enumerate(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations")):
            getattr(ev, name)[:chain.shape[1]] = chain[k + 1].astype(np.int64)
        ev.ptr = chain.shape[1]
        m.events = ev
        c = self.engine.counters(replicate)
        pos = (int(c.reserved[1]), 2 * int(c.reserved[2])) if c.reserved[1] >= 0 else None
        m.user_seed = int(self.seeds[replicate])
        return _capi.get_genealogy(m, seed, rng_position=pos)

    def genealogies(self, seed=None, replicates=None, layout='wave'):
        """The backward pass of every selected replicate of the last direct ``simulate(record_events=True)`` call at once,
        on the device (``vgx_get_genealogies``): one walk per replicate over its log where the kernel left it.  Returns a
        :class:`GenealogyBatch` whose ``replicate(r)`` is bit-identical to ``genealogy(r, seed_r)``.

        ``seed``: None (every replicate continues its own simulation stream), an int (every replicate reseeded with
        ``(seed, 0)``), or one seed per selected replicate.  ``replicates``: indices (default all, in order).  A replicate
        whose walk fails (fewer than two samples, lineages that never coalesce, ...) gets a nonzero status and does not
        fail the call.  ``layout``: 'wave' (one replicate per wavefront, the faster one measured) or 'lane'
        (one replicate per lane)."""
        if self._last_call is None:
            raise ValueError("genealogies() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("genealogies() walks direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("genealogies() needs the event log: the last call had record_events=False")
        if layout not in ('lane', 'wave'):
            raise ValueError("layout must be 'lane' or 'wave'")
        eng, lib = self.engine, self.engine.lib
        reps = np.arange(self.R, dtype=np.int64) if replicates is None else np.ascontiguousarray(replicates, dtype=np.int64).ravel()
        n = len(reps)
        if n and (reps.min() < 0 or reps.max() >= self.R):
            raise ValueError("replicate index out of range")
        if len(np.unique(reps)) != n:
            raise ValueError("replicates must be distinct")
        counters = [eng.counters(int(r)) for r in reps]
        for r, c in zip(reps, counters):
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started); use genealogy(r, seed)" % (r, c.ev_first_new))
        rng = self._walk_starts(reps, counters, seed)
        b = GenealogyBatch(reps)
        io = _capi.VgxGenealogiesIO()
        io.n = n
        io.replicates = _capi._p(reps)
        off = {k: np.zeros(n + 1, dtype=np.int64) for k in ("node", "mut", "mig")}
        io.node_off, io.mut_off, io.mig_off = _capi._p(off["node"]), _capi._p(off["mut"]), _capi._p(off["mig"])
        eng._check(lib.vgx_get_genealogies(eng.handle, C.byref(io)))          # sizing
        io.rng_state = rng.ctypes.data_as(C.POINTER(C.c_uint64))
        cap = {}
        for keys, o in ((GenealogyBatch.NODE_KEYS, off["node"]), (GenealogyBatch.MUT_KEYS, off["mut"]), (GenealogyBatch.MIG_KEYS, off["mig"])):
            for k in keys:
                cap[k] = np.zeros(max(int(o[-1]), 1), dtype=np.float64 if k.endswith("times") or k.endswith("_time") else np.int64)
        for k, a in cap.items():
            setattr(io, k, _capi._p(a))
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg", "nodes_used", "mut_n", "mig_n")}
        for k, a in per.items():
            setattr(io, k, _capi._p(a))
        rng_out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        io.rng_out = rng_out.ctypes.data_as(C.POINTER(C.c_uint64))
        io.layout = 1 if layout == 'wave' else 0
        eng._check(lib.vgx_get_genealogies(eng.handle, C.byref(io)))          # walk
        b._fill(off, cap, {k: v[:n] for k, v in per.items()}, rng_out[:n])
        b.passes, b.kernel_ms, b.clock_ms, b.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return b

    def _check_tau_genealogy_call(self, what):
        if self._last_call is None:
            raise ValueError("%s needs a simulate_tau(record_events=True) call first" % what)
        if self._last_call[0] != 'tau':
            raise ValueError("%s walks tau chains only: the last call was a direct simulate()" % what)
        if not self._last_call[1]:
            raise ValueError("%s needs the multievent rows: the last call had record_events=False" % what)

    def tau_genealogy(self, replicate, seed):
        """Backward pass (``GetGenealogy``, pyx:743-1000) over the WHOLE chain of one replicate of the last
        ``simulate_tau(record_events=True)`` call, on the host: the events and multievent rows the model held when the call
        started (none for a replicate that restarted), then the replicate's own steps with their rows in the reference's order
        (``_capi.canonical_multievents``), from the replicate's final state.  ``seed``: an int reseeds the stream with
        ``(seed, 0)``; None starts at ``(seeds[replicate], attempt 0, 0 draws)``, where the model's ``genealogy()`` starts after a
        tau call.  Returns the dict of ``_capi.get_genealogy``; a chain with a row the reference's pass cannot take (numpy's
        hypergeometric would raise on it) raises the text of the device pass's status 12 instead."""
        import copy
        self._check_tau_genealogy_call("tau_genealogy()")
        m = self._tau_chain_model(replicate)
        # vgx_get_genealogy trusts its rows as the reference does: where numpy's hypergeometric would raise (more migrants than the
        # source compartment holds, ...) or a transmission row draws more pairs than there are lineages, it reads and writes outside
        # its lists.  Tau steps at very small counts write such rows.  The guarded walk of the device pass (its host instance) goes
        # first on a copy of the counts: what it refuses is raised here with the device's text, and never reaches the host pass.
        probe = copy.copy(m)
        probe.infectious = m.infectious.copy()
        try:
            _capi.tau_genealogy_walk(probe, seed, rng_position=(0, 0))
        except RuntimeError as e:
            if str(e).startswith("vgx_get_tau_genealogies:"):
                raise
        return _capi.get_genealogy(m, seed, rng_position=(0, 0))

    def _tau_chain_model(self, replicate):
        """A host model with the final state and the WHOLE chain of one replicate of the last ``simulate_tau(record_events=True)``
        call, as ``tau_genealogy`` walks it: the model's events and rows before the call (none for a replicate that restarted),
        then the replicate's own steps with their rows in the reference's order.  A step of more rows than the device pass sorts
        raises its status-10 text."""
        from ._model import Events, MultiEvents
        eng = self.engine
        r = int(replicate)
        m = self.replicate_state(r)
        c = eng.counters(r)
        ev0, mv0, _ = self._tau_prefix
        if c.restarts > 0:
            n_pre, k_pre = 0, 0
        else:
            n_pre, k_pre = len(ev0[0]), len(mv0[0])
            if c.ev_first_new != n_pre:
                raise ValueError("replicate %d: its chain continues a log of %d events, the prefix holds %d" % (r, c.ev_first_new, n_pre))
        own = self.replicate_events(r)[:, int(c.ev_first_new):]
        starts, ends = own[2].astype(np.int64), own[3].astype(np.int64)
        if m.sCounter >= 2 and len(starts) and int((ends - starts).max()) > _capi.TAU_STEP_ROWS_MAX:   # what the device pass reports
            raise RuntimeError(_capi.genealogy_message(_capi.GW_STEP_ROWS, int(np.argmax(ends - starts > _capi.TAU_STEP_ROWS_MAX))))
        rows = _capi.canonical_multievents(eng.multievents(r), starts, ends, m.sites, m.susNum)
        n = n_pre + own.shape[1]
        ev = Events()
        ev.CreateEvents(max(n, 1))
        ev.times[:n] = np.concatenate((ev0[0][:n_pre], own[0]))
        for k, name in enumerate(ev.COLUMNS):
            col = own[k + 1].astype(np.int64)
            if name == "haplotypes":
                col = starts + k_pre                 # the MULTITYPE records' row ranges, behind the prefix's rows
            elif name == "populations":
                col = ends + k_pre
            getattr(ev, name)[:n] = np.concatenate((ev0[k + 1][:n_pre], col))
        ev.ptr = n
        mv = MultiEvents()
        mv.extend(np.concatenate((self._tau_prefix_mev_times[:k_pre], rows["times"])),
                  **{name: np.concatenate((mv0[j][:k_pre], rows[name])) for j, name in enumerate(mv.COLUMNS)})
        m.events, m.multievents = ev, mv
        m.user_seed = int(self.seeds[r])
        return m

    def _tau_genealogy_prefix_struct(self):
        """The model's chain before the last tau call as ``vgx_get_tau_genealogies`` and ``vgx_get_tau_lineages`` take it."""
        pre = _capi.VgxTauGenealogyPrefix()
        ev, mv, _ = self._tau_prefix
        pre.ev_ptr, pre.ev_times = len(ev[0]), _capi._p(ev[0])
        for name, col in zip(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations"), ev[1:]):
            setattr(pre, "ev_" + name, _capi._p(col))
        pre.mev_rows, pre.mev_times = len(mv[0]), _capi._p(self._tau_prefix_mev_times)
        for name, col in zip(_capi.MEV_COLUMNS, mv):
            setattr(pre, "mev_" + name, _capi._p(col))
        return pre

    def tau_genealogies(self, seed=None, replicates=None):
        """The backward pass of every selected replicate of the last ``simulate_tau(record_events=True)`` call at once, on the
        device (``vgx_get_tau_genealogies``): every step's rows are brought into the reference's order and granularity where the
        tau kernels left them (they are only read), then one walk per replicate over its whole chain: the model's chain before the
        call (shared, uploaded once; none for a replicate that restarted), then its own steps.  Returns a :class:`GenealogyBatch`
        whose ``replicate(r)`` equals ``tau_genealogy(r, seed_r)`` on every key, all six words of ``rng_raw`` included (the
        hypergeometric sampler's logarithm is the engine's own on the device and libm's on the host: a draw can differ only where
        a comparison is decided within the last ulp of a logarithm, include/vgx.h).

        ``seed`` and ``replicates`` as in ``genealogies()``; ``seed=None`` starts every walk at ``(seeds[r], attempt 0, 0
        draws)``.  A replicate whose walk fails (fewer than two samples, a step of more than 8192 raw rows, ...) gets a nonzero
        status and does not fail the call."""
        self._check_tau_genealogy_call("tau_genealogies()")
        eng, lib = self.engine, self.engine.lib
        reps = np.arange(self.R, dtype=np.int64) if replicates is None else np.ascontiguousarray(replicates, dtype=np.int64).ravel()
        n = len(reps)
        if n and (reps.min() < 0 or reps.max() >= self.R):
            raise ValueError("replicate index out of range")
        if len(np.unique(reps)) != n:
            raise ValueError("replicates must be distinct")
        if seed is not None and not np.isscalar(seed):
            seeds = np.ascontiguousarray(seed, dtype=np.int64).ravel()
            if len(seeds) != n:
                raise ValueError("one seed per selected replicate: got %d for %d" % (len(seeds), n))
        rng = np.zeros((max(n, 1), 6), dtype=np.uint64)
        pos = (C.c_uint64 * 4)()
        for i, r in enumerate(reps):
            lib.vgx_rng_position(int(self.seeds[r]) if seed is None else int(seed) if np.isscalar(seed) else int(seeds[i]), 0, 0, C.byref(pos))
            rng[i, :4] = list(pos)
        pre = self._tau_genealogy_prefix_struct()
        b = GenealogyBatch(reps)
        io = _capi.VgxTauGenealogiesIO()
        io.n = n
        io.replicates = _capi._p(reps)
        off = {k: np.zeros(n + 1, dtype=np.int64) for k in ("node", "mut", "mig")}
        io.node_off, io.mut_off, io.mig_off = _capi._p(off["node"]), _capi._p(off["mut"]), _capi._p(off["mig"])
        eng._check(lib.vgx_get_tau_genealogies(eng.handle, C.byref(io), C.byref(pre)))          # sizing
        io.rng_state = rng.ctypes.data_as(C.POINTER(C.c_uint64))
        cap = {}
        for keys, o in ((GenealogyBatch.NODE_KEYS, off["node"]), (GenealogyBatch.MUT_KEYS, off["mut"]), (GenealogyBatch.MIG_KEYS, off["mig"])):
            for k in keys:
                cap[k] = np.zeros(max(int(o[-1]), 1), dtype=np.float64 if k.endswith("times") or k.endswith("_time") else np.int64)
        for k, a in cap.items():
            setattr(io, k, _capi._p(a))
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg", "nodes_used", "mut_n", "mig_n")}
        for k, a in per.items():
            setattr(io, k, _capi._p(a))
        rng_out = np.zeros((max(n, 1), 6), dtype=np.uint64)
        io.rng_out = rng_out.ctypes.data_as(C.POINTER(C.c_uint64))
        eng._check(lib.vgx_get_tau_genealogies(eng.handle, C.byref(io), C.byref(pre)))          # walk
        b._fill(off, cap, {k: v[:n] for k, v in per.items()}, rng_out[:n])
        b.passes, b.kernel_ms, b.clock_ms, b.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return b

    def timelines(self, infectious=(), susceptible=(), step_num=100, replicates=None, semantics='reference'):
        """The log replays ``get_data_infectious(pop, hap, step_num)`` / ``get_data_susceptible(pop, group, step_num)``
        (pyx:1967-2045) of every selected replicate of the last direct ``simulate(record_events=True)`` call for a list of
        compartments at once, on the device (``vgx_get_timelines``): one pass per replicate over its log where the kernel left
        it.  Returns a :class:`TimelineBatch`.

        ``infectious``: ``(population, haplotype)`` pairs; ``susceptible``: ``(population, group)`` pairs (either may be empty;
        a pair given twice gets the same row twice).  ``replicates``: indices (default all, in order).  ``semantics``:
        'reference' is the reference's replay to the letter, including the operator precedence of pyx:1982 (a recovery or
        sampling in ANY compartment decrements every infectious series, every sampling counts in every ``Sample``) and zeros
        after the last grid index the replay reached; 'compartment' is the series of the compartment itself (births,
        recoveries, samplings, mutations out of and into it, migrations into it; ``Sample`` its own samplings), the value at
        the last reached index repeated after it: its ``Data[last_point]`` is the replicate's final state.  Every series
        starts from the replicate's ``initial_infectious`` / ``initial_susceptible``: for a model that had been simulated before and
        whose event log was empty when the ensemble started, that is not where the chain starts ('reference' still equals the
        reference's replay, 'compartment' then does not end in the final state).  Direct chains only: tau chains (MULTITYPE rows)
        are not replayed here."""
        if self._last_call is None:
            raise ValueError("timelines() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("timelines() replays direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("timelines() needs the event log: the last call had record_events=False")
        step_num, qi, ii, qs, si, reps = self._timeline_arguments(infectious, susceptible, step_num, replicates, semantics)
        eng = self.engine
        for r in reps:
            c = eng.counters(int(r))
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        return self._timeline_batch(lambda io: eng.lib.vgx_get_timelines(eng.handle, C.byref(io)), step_num, qi, ii, qs, si, reps, semantics)

    def tau_timelines(self, infectious=(), susceptible=(), step_num=100, replicates=None, semantics='reference'):
        """``timelines()`` for the replicates of the last ``simulate_tau(record_events=True)`` call (``vgx_get_tau_timelines``):
        the same queries, semantics, validation and :class:`TimelineBatch`, one pass per replicate over its multievent rows
        where the tau kernels left them.

        The reference replays the WHOLE chain of a model, so every replicate's series run over the events the model held when
        the tau call started (``model.events`` / ``model.multievents`` as they were then; shared by all replicates and uploaded
        once), followed by the replicate's own steps, on the grid ``i * currentTime_r / step_num`` of its own final time.  A
        replicate that restarted (``restarts > 0``) starts again at time 0 without that prefix.  Lockdown records: the model's
        before the call, then the replicate's (a restarted replicate: its own only).  Multievent rows take the rule of the
        reference's MULTITYPE branch (its susceptible MIGRATION clause tests ``haplotypes``, pyx:2037); 'compartment' keys the
        migrant's group where the tau kernels write it, so its ``Data[last_point]`` is ``replicate_states_tau()``'s state.  Series
        are exact while their values stay below 2^53 in magnitude."""
        if self._last_call is None:
            raise ValueError("tau_timelines() needs a simulate_tau(record_events=True) call first")
        if self._last_call[0] != 'tau':
            raise ValueError("tau_timelines() replays tau chains only: the last call was a direct simulate()")
        if not self._last_call[1]:
            raise ValueError("tau_timelines() needs the multievent rows: the last call had record_events=False")
        step_num, qi, ii, qs, si, reps = self._timeline_arguments(infectious, susceptible, step_num, replicates, semantics)
        eng = self.engine
        pre = self._tau_prefix_struct()
        return self._timeline_batch(lambda io: eng.lib.vgx_get_tau_timelines(eng.handle, C.byref(io), C.byref(pre)),
                                    step_num, qi, ii, qs, si, reps, semantics)

    def _tau_prefix_struct(self):
        """The ``vgx_timelines_prefix`` of the last ``simulate_tau(record_events=True)`` call: the model's events, multievent rows and
        lockdown records as they were when it started (the arrays live in ``self._tau_prefix``)."""
        pre = _capi.VgxTimelinesPrefix()
        ev, mv, loc = self._tau_prefix
        pre.ev_ptr, pre.ev_times = len(ev[0]), _capi._p(ev[0])
        for name, col in zip(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations"), ev[1:]):
            setattr(pre, "ev_" + name, _capi._p(col))
        pre.mev_rows = len(mv[0])
        for name, col in zip(_capi.MEV_COLUMNS, mv):
            setattr(pre, "mev_" + name, _capi._p(col))
        pre.loc_n, pre.loc_state, pre.loc_pop, pre.loc_time = len(loc[0]), _capi._p(loc[0]), _capi._p(loc[1]), _capi._p(loc[2])
        return pre

    def _timeline_arguments(self, infectious, susceptible, step_num, replicates, semantics):
        """The checks ``timelines()`` and ``tau_timelines()`` share: (step_num, unique infectious queries and the index of every given
        one among them, the same for the susceptible ones, replicates)."""
        if semantics not in _capi.TIMELINE_SEMANTICS:
            raise ValueError("semantics must be 'reference' or 'compartment'")
        step_num = int(step_num)
        if step_num < 1:
            raise ValueError("step_num must be at least 1")
        m = self.model
        qi, ii = _capi.unique_queries(infectious)
        qs, si = _capi.unique_queries(susceptible)
        for q, width, what in ((qi, m.hapNum, "haplotype"), (qs, m.susNum, "susceptibility group")):
            if len(q) and (q[:, 0].min() < 0 or q[:, 0].max() >= m.popNum):
                raise ValueError("population index out of range")
            if len(q) and (q[:, 1].min() < 0 or q[:, 1].max() >= width):
                raise ValueError("%s index out of range" % what)
        return step_num, qi, ii, qs, si, self._selected_replicates(replicates)

    def _timeline_batch(self, call, step_num, qi, ii, qs, si, reps, semantics):
        """The two-call protocol of ``vgx_get_timelines`` / ``vgx_get_tau_timelines`` (``call(io)`` returns the library's code)."""
        eng, n, T = self.engine, len(reps), step_num + 1
        io = _capi.VgxTimelinesIO()
        io.n, io.replicates, io.step_num, io.semantics = n, _capi._p(reps), step_num, _capi.TIMELINE_SEMANTICS[semantics]
        keep = [np.ascontiguousarray(q[:, j]) for q in (qi, qs) for j in (0, 1)]
        io.n_inf, io.inf_pop, io.inf_hap = len(qi), _capi._p(keep[0]), _capi._p(keep[1])
        io.n_sus, io.sus_pop, io.sus_grp = len(qs), _capi._p(keep[2]), _capi._p(keep[3])
        eng._check(call(io))                                                  # sizing
        cap = int(io.loc_cap)
        tp = np.zeros((max(n, 1), T))
        inf, smp = np.zeros((max(n, 1), max(len(qi), 1), T)), np.zeros((max(n, 1), max(len(qi), 1), T))
        sus = np.zeros((max(n, 1), max(len(qs), 1), T))
        if len(qi) == 0:
            inf, smp = inf[:, :0], smp[:, :0]
        if len(qs) == 0:
            sus = sus[:, :0]
        last, loc_n = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        loc_state, loc_pop = np.zeros((max(n, 1), cap), dtype=np.int64), np.zeros((max(n, 1), cap), dtype=np.int64)
        loc_time = np.zeros((max(n, 1), cap))
        io.time_points, io.last_point = _capi._p(tp), _capi._p(last)
        io.inf_data = _capi._p(inf) if len(qi) else None
        io.inf_sample = _capi._p(smp) if len(qi) else None
        io.sus_data = _capi._p(sus) if len(qs) else None
        io.loc_n, io.loc_state, io.loc_pop, io.loc_time = _capi._p(loc_n), _capi._p(loc_state), _capi._p(loc_pop), _capi._p(loc_time)
        eng._check(call(io))                                                  # replay
        b = TimelineBatch(reps, qi[ii], qs[si], step_num, semantics)
        b.time_points, b.last_point = tp[:n], last[:n]
        b.infectious, b.samples, b.susceptible = inf[:n][:, ii], smp[:n][:, ii], sus[:n][:, si]
        b._loc = (loc_n[:n], loc_state[:n], loc_pop[:n], loc_time[:n])
        b.passes, b.kernel_ms, b.clock_ms, b.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return b

    def _selected_replicates(self, replicates):
        """``replicates`` as an int64 array of distinct indices (default all, in order); ValueError otherwise."""
        reps = np.arange(self.R, dtype=np.int64) if replicates is None else np.ascontiguousarray(replicates, dtype=np.int64).ravel()
        if len(reps) and (reps.min() < 0 or reps.max() >= self.R):
            raise ValueError("replicate index out of range")
        if len(np.unique(reps)) != len(reps):
            raise ValueError("replicates must be distinct")
        return reps

    def _block_summary(self, summary, reps, cols, scenario_of, n_scenarios, leave_out=None):
        """The ``summary=`` dict of ``incidence()``, ``tau_incidence()``, ``prevalence()`` and ``tau_prevalence()`` checked and turned into the
        (io, finish) of ``_summary_request`` over the selected replicates' block with columns of the shape ``cols``;
        (None, None) without one.  ``leave_out`` [R] bool: replicates that are in no group, whatever ``by`` says."""
        if summary is None:
            return None, None
        unknown = set(summary) - {"quantiles", "by", "method"}
        if unknown:
            raise ValueError("summary takes quantiles, by and method: got %s" % ", ".join(sorted(unknown)))
        method = summary.get("method", 'linear')
        q = _summary_quantiles(summary.get("quantiles", (0.025, 0.5, 0.975)), method)
        group_of, G = _summary_groups(summary.get("by", 'auto'), None, self.R, scenario_of, n_scenarios)
        if leave_out is not None:
            group_of[leave_out] = -1
        return _summary_request(np.ascontiguousarray(group_of[reps]), G, q, method, cols)

    def _incidence_request(self, io, e, replicates, haplotypes, summary, counts, dtype, scenario_of, n_scenarios):
        """What ``incidence()`` and ``tau_incidence()`` share: the checks on ``replicates``, ``haplotypes``, ``summary`` and ``counts``
        (ValueError before the library is called) and the fields both io structures have.  Returns ``finish(check)``, which the caller
        invokes after its own checks: ``check()`` makes the library call; the result is the :class:`Incidence`."""
        m = self.model
        reps = self._selected_replicates(replicates)
        n = len(reps)
        mask = None if haplotypes is None else _capi.haplotype_mask(haplotypes, m.hapNum)
        T, P, K = len(e) - 1, m.popNum, len(Incidence.CHANNELS)
        sio, done = self._block_summary(summary, reps, (T, P, K), scenario_of, n_scenarios)
        if summary is None and not counts:
            raise ValueError("counts=False needs summary=: the call would return nothing")
        block = np.zeros((n, T, P, K), dtype=dtype) if counts else None
        outside = np.zeros((max(n, 1), 2), dtype=np.int64)
        io.n, io.replicates, io.T, io.edges = n, _capi._p(reps), T, _capi._p(e)
        io.hap_mask = None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint32))
        io.counts = block.ctypes.data_as(type(io.counts)) if counts and n else None
        io.outside = _capi._p(outside)
        io.summary = C.pointer(sio) if sio is not None and n else None

        def finish(check, _alive=(reps, mask, e)):
            check()
            inc = Incidence()
            inc.counts, inc.edges, inc.outside, inc.replicates = block, e, outside[:n], reps
            inc.summary = done() if done is not None else None
            inc.passes, inc.kernel_ms, inc.clock_ms, inc.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
            return inc
        return finish

    def incidence(self, edges=None, bins=None, window=None, replicates=None, haplotypes=None, summary=None, counts=True):
        """Event counts per time bin, population and channel of every selected replicate of the last direct
        ``simulate(record_events=True)`` call, on ONE grid for all replicates and on the device (``vgx_get_incidence``): one
        streaming pass over every replicate's log where the kernel left it.  Returns an :class:`Incidence`.

        The grid: ``edges`` [T + 1] strictly increasing, or ``bins`` and ``window=(t0, t1)``, which form
        ``edges[k] = t0 + (k (t1 - t0)) / bins`` with ``edges[bins] = t1``.  Bin b holds the events with
        ``edges[b] <= t < edges[b + 1]``.  ``replicates``: indices (default all, in order).  ``haplotypes``: indices of the
        haplotypes to count (default all): a birth, death, sampling or migration counts if its haplotype is among them, a
        mutation if the variant that arises is; immunity changes carry no haplotype and are not counted under a filter.
        ``summary``: a dict of ``quantiles``, ``by`` and ``method`` as ``trajectory_summary`` takes them: the counts are
        summarised across the selected replicates in the same call, where they lie (``by='auto'``: one group per scenario of a
        scenario ensemble); with ``counts=False`` the block itself is not copied to the host.  Direct chains only."""
        e = _incidence_edges(edges, bins, window)
        if self._last_call is None:
            raise ValueError("incidence() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("incidence() counts direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("incidence() needs the event log: the last call had record_events=False")
        io = _capi.VgxIncidenceIO()
        finish = self._incidence_request(io, e, replicates, haplotypes, summary, counts, np.int32, self.scenario_of,
                                         len(self.scenarios) if self.scenarios is not None else 1)
        eng = self.engine
        for r in range(io.n):
            c = eng.counters(int(io.replicates[r]))
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (io.replicates[r], c.ev_first_new))
        return finish(lambda: eng._check(eng.lib.vgx_get_incidence(eng.handle, C.byref(io))))

    def tau_incidence(self, edges=None, bins=None, window=None, replicates=None, haplotypes=None, summary=None, counts=True):
        """``incidence()`` for the replicates of the last ``simulate_tau(record_events=True)`` call (``vgx_get_tau_incidence``): the
        same grid arguments, channels, haplotype filter, ``summary`` and :class:`Incidence`, with ``counts`` [n, T, P, 7] int64 (a
        bin sums the multiplicities of many steps) and ``outside`` the summed multiplicities before and after the window.

        A replicate's chain is the model's chain before the tau call (``model.events`` / ``model.multievents`` as they were
        then; a replicate that restarted has none), then its own steps, every multievent row counting ``num`` times.  All events
        of a step carry the time of the step's MULTITYPE record, which is where the reference's own replays place them, so a
        step falls into one bin whole.  The shared part is counted once per call on the device, not once per replicate; no
        host clock runs.  ``summary``: refused by the library when a count reaches 2^31 (``counts`` stays available: call
        again without ``summary``).  ``by='auto'``: one group per scenario of a scenario ensemble."""
        e = _incidence_edges(edges, bins, window)
        if self._last_call is None:
            raise ValueError("tau_incidence() needs a simulate_tau(record_events=True) call first")
        if self._last_call[0] != 'tau':
            raise ValueError("tau_incidence() counts tau chains only: the last call was a direct simulate()")
        if not self._last_call[1]:
            raise ValueError("tau_incidence() needs the multievent rows: the last call had record_events=False")
        io = _capi.VgxTauIncidenceIO()
        finish = self._incidence_request(io, e, replicates, haplotypes, summary, counts, np.int64, *self._scenario_groups())
        eng, pre = self.engine, self._tau_prefix_struct()
        return finish(lambda: eng._check(eng.lib.vgx_get_tau_incidence(eng.handle, C.byref(io), C.byref(pre))))

    def flows(self, edges=None, bins=None, window=None, variants=None, within=True, replicates=None, summary=None, counts=True):
        """Who infects whom: new infections per time bin, source population, destination population and variant class of every
        selected replicate of the last direct ``simulate(record_events=True)`` call, on ONE grid for all replicates and on the
        device (``vgx_get_flows``): one streaming pass over every replicate's log where the kernel left it.  Returns a
        :class:`Flows`.

        Every new infection in the log names its source: a birth in p is a transmission within p and counts at
        ``[src, dst] = [p, p]``, a migration is a transmission across and counts at ``[population, newPopulation]``.
        ``within=False`` leaves the births out.  The grid as ``incidence()`` takes it: ``edges`` [T + 1], or ``bins`` and
        ``window=(t0, t1)``.  ``variants`` as ``prevalence()`` takes them: None (every haplotype its own class), an integer
        array [H] of classes with -1 for haplotypes that are not tracked, or a sequence of sequences of haplotype indices; a new
        infection counts in the class of its haplotype.  ``replicates``, ``summary`` and ``counts=False`` as in ``incidence()``.
        With ``haplotypes`` = the members of class c, ``incidence()``'s channels are this block's margins: births the diagonal,
        arrivals the off-diagonal sum over src, departures the off-diagonal sum over dst.  Direct chains only."""
        e = _incidence_edges(edges, bins, window)
        if self._last_call is None:
            raise ValueError("flows() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("flows() counts direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("flows() needs the event log: the last call had record_events=False")
        m, eng = self.model, self.engine
        reps = self._selected_replicates(replicates)
        n = len(reps)
        vo, V = _capi.variant_map(variants, m.hapNum)
        T, P = len(e) - 1, m.popNum
        if 4 * P * V > 65536:
            raise ValueError("%d populations x %d classes need %d bytes of cells, above the 65536 bytes of LDS a counting workgroup may use"
                             % (P, V, 4 * P * V))
        sio, done = self._block_summary(summary, reps, (T, P, P, V), self.scenario_of, len(self.scenarios) if self.scenarios is not None else 1)
        if summary is None and not counts:
            raise ValueError("counts=False needs summary=: the call would return nothing")
        for r in reps:
            c = eng.counters(int(r))
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        block = np.zeros((n, T, P, P, V), dtype=np.int32) if counts else None
        outside = np.zeros((max(n, 1), 2), dtype=np.int64)
        i32 = C.POINTER(C.c_int32)
        io = _capi.VgxFlowsIO()
        io.n, io.replicates, io.T, io.edges, io.V, io.variant_of = n, _capi._p(reps), T, _capi._p(e), V, vo.ctypes.data_as(i32)
        io.within = 1 if within else 0
        io.counts = block.ctypes.data_as(i32) if counts and n else None
        io.outside = _capi._p(outside)
        io.summary = C.pointer(sio) if sio is not None and n else None
        eng._check(eng.lib.vgx_get_flows(eng.handle, C.byref(io)))
        fl = Flows()
        fl.counts, fl.edges, fl.variant_of, fl.outside, fl.replicates = block, e, vo, outside[:n], reps
        fl.summary = done() if done is not None else None
        fl.form = _capi.FLOW_FORM_NAMES[int(io.form)]
        fl.passes, fl.kernel_ms, fl.clock_ms, fl.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return fl

    def tau_flows(self, edges=None, bins=None, window=None, variants=None, within=True, replicates=None, summary=None, counts=True):
        """``flows()`` for the replicates of the last ``simulate_tau(record_events=True)`` call (``vgx_get_tau_flows``): the same
        grid arguments, ``variants``, ``within``, ``replicates``, ``summary`` and :class:`Flows`, with ``counts``
        [n, T, P, P, V] int64 (a bin sums the multiplicities of many steps) and ``outside`` the summed multiplicities before and
        after the window.

        The chain is ``tau_incidence()``'s: the model's chain before the tau call (a replicate that restarted has none), then
        the replicate's own steps, every multievent row counting ``num`` times in the one cell ``flows()`` gives it; all events
        of a step fall into the bin of the step's MULTITYPE record.  The shared part is counted once per call on the device; no
        host clock runs.  With ``haplotypes`` = the members of class c, ``tau_incidence()``'s channels are this block's margins.
        ``summary``: refused by the library when a count reaches 2^31 (``counts`` stays available: call again without
        ``summary``).  ``by='auto'``: one group per scenario of a scenario ensemble."""
        e = _incidence_edges(edges, bins, window)
        if self._last_call is None:
            raise ValueError("tau_flows() needs a simulate_tau(record_events=True) call first")
        if self._last_call[0] != 'tau':
            raise ValueError("tau_flows() counts tau chains only: the last call was a direct simulate()")
        if not self._last_call[1]:
            raise ValueError("tau_flows() needs the multievent rows: the last call had record_events=False")
        m, eng = self.model, self.engine
        reps = self._selected_replicates(replicates)
        n = len(reps)
        vo, V = _capi.variant_map(variants, m.hapNum)
        T, P = len(e) - 1, m.popNum
        _capi.tau_flows_lds_check(P, V)
        sio, done = self._block_summary(summary, reps, (T, P, P, V), *self._scenario_groups())
        if summary is None and not counts:
            raise ValueError("counts=False needs summary=: the call would return nothing")
        block = np.zeros((n, T, P, P, V), dtype=np.int64) if counts else None
        outside = np.zeros((max(n, 1), 2), dtype=np.int64)
        io = _capi.VgxTauFlowsIO()
        io.n, io.replicates, io.T, io.edges = n, _capi._p(reps), T, _capi._p(e)
        io.V, io.variant_of = V, vo.ctypes.data_as(C.POINTER(C.c_int32))
        io.within = 1 if within else 0
        io.counts = _capi._p(block) if counts and n else None
        io.outside = _capi._p(outside)
        io.summary = C.pointer(sio) if sio is not None and n else None
        pre = self._tau_prefix_struct()
        eng._check(eng.lib.vgx_get_tau_flows(eng.handle, C.byref(io), C.byref(pre)))
        fl = Flows()
        fl.counts, fl.edges, fl.variant_of, fl.outside, fl.replicates = block, e, vo, outside[:n], reps
        fl.summary = done() if done is not None else None
        fl.form = _capi.FLOW_FORM_NAMES[int(io.form)]
        fl.passes, fl.kernel_ms, fl.clock_ms, fl.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return fl

    def prevalence(self, times=None, points=None, window=None, variants=None, replicates=None, summary=None, values=True):
        """Infectious hosts per grid time, population and variant class of every selected replicate of the last direct
        ``simulate(record_events=True)`` call, on ONE grid for all replicates and on the device (``vgx_get_prevalence``): a
        tile-parallel pass over every replicate's log where the kernel left it forms the net change per interval, a scan sums
        the intervals up.  Returns a :class:`Prevalence`.

        The grid: ``times`` [T] strictly increasing, or ``points`` and ``window=(t0, t1)``, which form
        ``t0 + j ((t1 - t0) / (points - 1))``, the grid of ``simulate(traj_points=, traj_window=)`` (``points=1``: ``[t0]``).  A
        grid time gets the state with every event up to and including that time applied, as the trajectories do.
        ``variants``: None (every haplotype its own class), an integer array [H] of classes with -1 for haplotypes that are not
        tracked, or a sequence of sequences of haplotype indices (class k = the k-th sequence, the rest not tracked).
        ``replicates``: indices (default all, in order).  ``summary``: a dict of ``quantiles``, ``by`` and ``method`` as
        ``trajectory_summary`` takes them: the values are summarised across the selected replicates in the same call, where
        they lie (``by='auto'``: one group per scenario of a scenario ensemble); with ``values=False`` the block itself is not
        copied to the host.  Direct chains only."""
        g = _prevalence_grid(times, points, window)
        if self._last_call is None:
            raise ValueError("prevalence() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("prevalence() counts direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("prevalence() needs the event log: the last call had record_events=False")
        eng = self.engine
        reps, n, vo, V, T, P, sio, done = self._prevalence_request(g, variants, replicates, summary, values, 4, self.scenario_of,
                                                                   len(self.scenarios) if self.scenarios is not None else 1)
        for r in reps:
            c = eng.counters(int(r))
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        block = np.zeros((n, T, P, V), dtype=np.int32) if values else None
        final = np.zeros((n, P, V), dtype=np.int32)
        outside = np.zeros((max(n, 1), 2), dtype=np.int64)
        i32 = C.POINTER(C.c_int32)
        io = _capi.VgxPrevalenceIO()
        io.n, io.replicates, io.T, io.grid, io.V, io.variant_of = n, _capi._p(reps), T, _capi._p(g), V, vo.ctypes.data_as(i32)
        io.values = block.ctypes.data_as(i32) if values and n else None
        io.final = final.ctypes.data_as(i32) if n else None
        io.outside = _capi._p(outside)
        io.summary = C.pointer(sio) if sio is not None and n else None
        eng._check(eng.lib.vgx_get_prevalence(eng.handle, C.byref(io)))
        pv = Prevalence()
        pv.values, pv.final, pv.times, pv.variant_of, pv.outside, pv.replicates = block, final, g, vo, outside[:n], reps
        pv.summary = done() if done is not None else None
        pv.passes, pv.kernel_ms, pv.clock_ms, pv.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return pv

    def _walk_starts(self, reps, counters, seed):
        """The generator start of every selected replicate's backward walk, [n, 4] uint64, as ``genealogy(r, seed)`` finds it:
        ``seed`` None (the replicate continues its own simulation stream), an int, or one seed per selected replicate."""
        lib, n = self.engine.lib, len(reps)
        if seed is not None and not np.isscalar(seed):
            seeds = np.ascontiguousarray(seed, dtype=np.int64).ravel()
            if len(seeds) != n:
                raise ValueError("one seed per selected replicate: got %d for %d" % (len(seeds), n))
        rng = np.zeros((max(n, 1), 4), dtype=np.uint64)
        pos = (C.c_uint64 * 4)()
        for i, (r, c) in enumerate(zip(reps, counters)):
            if seed is None:
                att, draws = (int(c.reserved[1]), 2 * int(c.reserved[2])) if c.reserved[1] >= 0 else (0, 0)
                lib.vgx_rng_position(int(self.seeds[r]), att, draws, C.byref(pos))
            else:
                lib.vgx_rng_position(int(seed) if np.isscalar(seed) else int(seeds[i]), 0, 0, C.byref(pos))
            rng[i] = list(pos)
        return rng

    def lineages(self, times=None, points=None, window=None, variants=None, seed=None, replicates=None, summary=None, values=True):
        """Ancestral lineages of the sampled cases per grid time, population and variant class of every selected replicate of the
        last direct ``simulate(record_events=True)`` call, on ONE grid for all replicates and on the device
        (``vgx_get_lineages``): the lineages-through-time curve of every replicate's tree, structured by population and variant.
        The walk is that of ``genealogies(seed, replicates)``, with the same draws, status and generator afterwards, and logs
        where it changes a lineage list (also where a migration moves a lineage without coalescing, and the haplotype a lineage
        carries, neither of which ``genealogies()`` returns); a tile-parallel pass bins the logs on the grid and a scan sums the
        intervals up.  Returns a :class:`Lineages`.

        The grid (``times``, or ``points`` and ``window``) and ``variants`` as ``prevalence()`` takes them; ``seed`` and
        ``replicates`` as ``genealogies()``.  A replicate whose walk fails (fewer than two samples, lineages that never coalesce,
        ...) gets its status and zeros and does not fail the call.  ``summary``: a dict of ``quantiles``, ``by`` and ``method`` as
        ``trajectory_summary`` takes them; replicates with fewer than two samples are left out of its groups, any other failed
        walk inside a group refuses the summary (after the values are there: the exception carries them as ``.lineages``); with
        ``values=False`` the block itself is not copied to the host.  Direct chains only."""
        g = _prevalence_grid(times, points, window)
        if self._last_call is None:
            raise ValueError("lineages() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("lineages() walks direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("lineages() needs the event log: the last call had record_events=False")
        eng = self.engine
        reps = self._selected_replicates(replicates)
        counters = [eng.counters(int(r)) for r in reps]
        for r, c in zip(reps, counters):
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        rng = self._walk_starts(reps, counters, seed)
        # replicates with fewer than two samples are known from the counters before any walk: they are in no group of the summary
        few = np.zeros(self.R, dtype=bool)
        few[reps] = [c.reserved[4] < 2 for c in counters]
        reps, n, vo, V, T, P, sio, done = self._prevalence_request(g, variants, reps, summary, values, 4, self.scenario_of,
                                                                   len(self.scenarios) if self.scenarios is not None else 1, leave_out=few)
        block = np.zeros((n, T, P, V), dtype=np.int32) if values else None
        root = np.zeros((max(n, 1), P, V), dtype=np.int32)
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg", "records")}
        rng_out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        i32, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
        io = _capi.VgxLineagesIO()
        io.n, io.replicates, io.rng_state = n, _capi._p(reps), rng.ctypes.data_as(u64)
        io.T, io.grid, io.V, io.variant_of = T, _capi._p(g), V, vo.ctypes.data_as(i32)
        io.values = block.ctypes.data_as(i32) if values and n else None
        io.root = root.ctypes.data_as(i32)
        io.status, io.status_arg, io.records = _capi._p(per["status"]), _capi._p(per["status_arg"]), _capi._p(per["records"])
        io.rng_out = rng_out.ctypes.data_as(u64)
        io.summary = C.pointer(sio) if sio is not None and n else None
        rc = eng.lib.vgx_get_lineages(eng.handle, C.byref(io))
        ln = Lineages()
        ln.values, ln.root, ln.times, ln.variant_of, ln.replicates = block, root[:n], g, vo, reps
        ln.status, ln.status_arg, ln.records = per["status"][:n], per["status_arg"][:n], per["records"][:n]
        ln.rng_raw = np.zeros((n, 6), dtype=np.uint64)
        ln.rng_raw[:, :4] = rng_out[:n]
        ln.summary = None
        ln.passes, ln.kernel_ms, ln.clock_ms, ln.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        ln.stage_ms = tuple(io.kernel_ms)
        try:
            eng._check(rc)
        except _capi.VgxError as err:
            if sio is not None and ": summary: " in str(err):   # refused after values, root and status were delivered
                err.lineages = ln
            raise
        ln.summary = done() if done is not None else None
        return ln

    def tau_lineages(self, times=None, points=None, window=None, variants=None, seed=None, replicates=None, summary=None, values=True):
        """``lineages()`` for the replicates of the last ``simulate_tau(record_events=True)`` call (``vgx_get_tau_lineages``): the
        lineages-through-time curve of every tau replicate's tree, structured by population and variant, on ONE grid and on the
        device.  The walk is that of ``tau_genealogies(seed, replicates)`` over the same chain (the model's chain before the
        call, none for a replicate that restarted, then the replicate's own steps in the reference's row order), with the same
        draws, status and six generator words afterwards; it logs where a row changes a lineage list, and the binning and
        suffix-sum passes of ``lineages()`` turn the logs into the block.  All rows of a step share the step's time: a grid time
        exactly at a step's time has the whole step applied, as ``tau_prevalence()`` has it.  Returns a :class:`Lineages`
        (``stage_ms``: the canonicalise, walk, binning and suffix-sum kernels apart), so ``sampled_share(tau_prevalence(...))`` on
        the same grid, replicates and variants works.

        The grid, ``variants``, ``summary`` and ``values`` as ``lineages()``; ``seed`` and ``replicates`` as
        ``tau_genealogies()`` (``seed=None`` starts every walk at ``(seeds[r], attempt 0, 0 draws)``).  A replicate whose walk
        fails (fewer than two samples, a step of more than 8192 raw rows, ...) gets its status and zeros and does not fail the
        call; replicates with fewer than two samples are left out of the summary's groups, any other failed walk inside a group
        refuses the summary after the values are there (the exception carries them as ``.lineages``)."""
        g = _prevalence_grid(times, points, window)
        self._check_tau_genealogy_call("tau_lineages()")
        eng, lib = self.engine, self.engine.lib
        reps = self._selected_replicates(replicates)
        n = len(reps)
        if seed is not None and not np.isscalar(seed):
            seeds = np.ascontiguousarray(seed, dtype=np.int64).ravel()
            if len(seeds) != n:
                raise ValueError("one seed per selected replicate: got %d for %d" % (len(seeds), n))
        rng = np.zeros((max(n, 1), 6), dtype=np.uint64)
        pos = (C.c_uint64 * 4)()
        for i, r in enumerate(reps):
            lib.vgx_rng_position(int(self.seeds[r]) if seed is None else int(seed) if np.isscalar(seed) else int(seeds[i]), 0, 0, C.byref(pos))
            rng[i, :4] = list(pos)
        few = None
        if summary is not None:   # replicates with fewer than two samples are known from the counters before any walk: they are in no group
            few = np.zeros(self.R, dtype=bool)
            few[reps] = [eng.counters(int(r)).reserved[4] < 2 for r in reps]
        reps, n, vo, V, T, P, sio, done = self._prevalence_request(g, variants, reps, summary, values, 4, self.scenario_of,
                                                                   len(self.scenarios) if self.scenarios is not None else 1, leave_out=few)
        pre = self._tau_genealogy_prefix_struct()
        block = np.zeros((n, T, P, V), dtype=np.int32) if values else None
        root = np.zeros((max(n, 1), P, V), dtype=np.int32)
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg", "records")}
        rng_out = np.zeros((max(n, 1), 6), dtype=np.uint64)
        i32, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
        io = _capi.VgxTauLineagesIO()
        io.n, io.replicates, io.rng_state = n, _capi._p(reps), rng.ctypes.data_as(u64)
        io.T, io.grid, io.V, io.variant_of = T, _capi._p(g), V, vo.ctypes.data_as(i32)
        io.values = block.ctypes.data_as(i32) if values and n else None
        io.root = root.ctypes.data_as(i32)
        io.status, io.status_arg, io.records = _capi._p(per["status"]), _capi._p(per["status_arg"]), _capi._p(per["records"])
        io.rng_out = rng_out.ctypes.data_as(u64)
        io.summary = C.pointer(sio) if sio is not None and n else None
        rc = lib.vgx_get_tau_lineages(eng.handle, C.byref(io), C.byref(pre))
        ln = Lineages()
        ln.values, ln.root, ln.times, ln.variant_of, ln.replicates = block, root[:n], g, vo, reps
        ln.status, ln.status_arg, ln.records = per["status"][:n], per["status_arg"][:n], per["records"][:n]
        ln.rng_raw = rng_out[:n]
        ln.summary = None
        ln.passes, ln.kernel_ms, ln.clock_ms, ln.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        ln.stage_ms = tuple(io.kernel_ms)
        try:
            eng._check(rc)
        except _capi.VgxError as err:
            if sio is not None and ": summary: " in str(err):   # refused after values, root and status were delivered
                err.lineages = ln
            raise
        ln.summary = done() if done is not None else None
        return ln

    def tree_events(self, times=None, points=None, window=None, variants=None, seed=None, replicates=None, summary=None, values=True):
        """The events of every selected replicate's sampled tree per interval of ONE grid, population, variant class and kind, for
        the last direct ``simulate(record_events=True)`` call and on the device (``vgx_get_tree_events``): samples, coalescences
        (the skyline's numerator), lineage mutations within and between classes, and lineage moves out of and into every
        population.  The walk and its lineage log are those of ``lineages()``; one binning pass keeps the kinds apart.  Returns a
        :class:`TreeEvents`, whose ``lineages()`` gives what ``lineages()`` returns for the same arguments without a second walk.

        All arguments as ``lineages()`` takes them, with its refusals; interval i = 0 .. T of the block lies between
        ``times[i - 1]`` and ``times[i]`` (the last one after ``times[-1]``).  ``summary`` is taken over the [T + 1, P, V, 7] columns;
        a summary refused after the block is there carries it as ``.tree_events``.  Direct chains only."""
        g = _prevalence_grid(times, points, window)
        if self._last_call is None:
            raise ValueError("tree_events() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("tree_events() walks direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("tree_events() needs the event log: the last call had record_events=False")
        reps = self._selected_replicates(replicates)
        counters = [self.engine.counters(int(r)) for r in reps]
        for r, c in zip(reps, counters):
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        rng = self._walk_starts(reps, counters, seed)
        return self._tree_events(False, g, variants, reps, rng, [c.reserved[4] < 2 for c in counters], summary, values)

    def tau_tree_events(self, times=None, points=None, window=None, variants=None, seed=None, replicates=None, summary=None, values=True):
        """``tree_events()`` for the replicates of the last ``simulate_tau(record_events=True)`` call
        (``vgx_get_tau_tree_events``): the walk, chain and cuts of ``tau_lineages()`` with the binning of ``tree_events()``.  All
        records of a step share the step's time: a grid time exactly at a step's time has the whole step in the intervals up to
        it.  Arguments and refusals as ``tau_lineages()``; returns a :class:`TreeEvents` (``stage_ms``: canonicalise, walk,
        binning)."""
        g = _prevalence_grid(times, points, window)
        self._check_tau_genealogy_call("tau_tree_events()")
        lib = self.engine.lib
        reps = self._selected_replicates(replicates)
        n = len(reps)
        if seed is not None and not np.isscalar(seed):
            seeds = np.ascontiguousarray(seed, dtype=np.int64).ravel()
            if len(seeds) != n:
                raise ValueError("one seed per selected replicate: got %d for %d" % (len(seeds), n))
        rng = np.zeros((max(n, 1), 6), dtype=np.uint64)
        pos = (C.c_uint64 * 4)()
        for i, r in enumerate(reps):
            lib.vgx_rng_position(int(self.seeds[r]) if seed is None else int(seed) if np.isscalar(seed) else int(seeds[i]), 0, 0, C.byref(pos))
            rng[i, :4] = list(pos)
        few = [self.engine.counters(int(r)).reserved[4] < 2 for r in reps] if summary is not None else None
        return self._tree_events(True, g, variants, reps, rng, few, summary, values)

    def _tree_events(self, tau, g, variants, reps, rng, few, summary, values):
        """What ``tree_events()`` and ``tau_tree_events()`` share once the walks' starts ``rng`` are known: the checks on
        ``variants``, the LDS limit, ``summary`` and ``values``, the library call and the :class:`TreeEvents`.  ``few``: per selected
        replicate, fewer than two samples (known from the counters before any walk: such a replicate is in no group)."""
        eng = self.engine
        vo, V = _capi.variant_map(variants, self.model.hapNum)
        n, T, P, K = len(reps), len(g), self.model.popNum, len(TreeEvents.CHANNELS)
        if 4 * K * P * V > 65536:
            raise ValueError("%d populations x %d classes x %d channels need %d bytes of cells, above the 65536 bytes of LDS a counting "
                             "workgroup may use" % (P, V, K, 4 * K * P * V))
        leave_out = None
        if few is not None:
            leave_out = np.zeros(self.R, dtype=bool)
            leave_out[reps] = few
        sio, done = self._block_summary(summary, reps, (T + 1, P, V, K), self.scenario_of,
                                        len(self.scenarios) if self.scenarios is not None else 1, leave_out)
        if summary is None and not values:
            raise ValueError("values=False needs summary=: the call would return nothing")
        words = 6 if tau else 4
        block = np.zeros((n, T + 1, P, V, K), dtype=np.int32) if values else None
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg", "records")}
        rng_out = np.zeros((max(n, 1), words), dtype=np.uint64)
        i32, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
        io = _capi.VgxTauTreeEventsIO() if tau else _capi.VgxTreeEventsIO()
        io.n, io.replicates, io.rng_state = n, _capi._p(reps), rng.ctypes.data_as(u64)
        io.T, io.grid, io.V, io.variant_of = T, _capi._p(g), V, vo.ctypes.data_as(i32)
        io.counts = block.ctypes.data_as(i32) if values and n else None
        io.status, io.status_arg, io.records = _capi._p(per["status"]), _capi._p(per["status_arg"]), _capi._p(per["records"])
        io.rng_out = rng_out.ctypes.data_as(u64)
        io.summary = C.pointer(sio) if sio is not None and n else None
        if tau:
            pre = self._tau_genealogy_prefix_struct()
            rc = eng.lib.vgx_get_tau_tree_events(eng.handle, C.byref(io), C.byref(pre))
        else:
            rc = eng.lib.vgx_get_tree_events(eng.handle, C.byref(io))
        te = TreeEvents()
        te.counts, te.times, te.variant_of, te.replicates = block, g, vo, reps
        te.status, te.status_arg, te.records = per["status"][:n], per["status_arg"][:n], per["records"][:n]
        te.rng_raw = np.zeros((n, 6), dtype=np.uint64)
        te.rng_raw[:, :words] = rng_out[:n]
        te.summary = None
        te.passes, te.kernel_ms, te.clock_ms, te.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        te.stage_ms = tuple(io.kernel_ms)
        try:
            eng._check(rc)
        except _capi.VgxError as err:
            if sio is not None and ": summary: " in str(err):   # refused after counts and status were delivered
                err.tree_events = te
            raise
        te.summary = done() if done is not None else None
        return te

    def tree_shapes(self, seed=None, replicates=None):
        """Balance, depth and branch statistics of the sampled tree of every selected replicate of the last direct
        ``simulate(record_events=True)`` call, on the device (``vgx_get_tree_shapes``): the walk of ``genealogies(seed, replicates)``
        with the same draws, status and generator afterwards, then one kernel that reduces every tree where the walk left it to a
        row of 12 integers and 7 lengths; only the node event indices and the node times cross to the host and back.  Returns a
        :class:`TreeShapes`, whose rows are what the tree of ``genealogies(seed).replicate(r)`` gives.

        ``seed`` and ``replicates`` as ``genealogies()``.  A replicate whose walk fails (fewer than two samples, lineages that never
        coalesce, ...) gets its status, zeros and NaN and does not fail the call.  Direct chains only."""
        if self._last_call is None:
            raise ValueError("tree_shapes() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("tree_shapes() walks direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("tree_shapes() needs the event log: the last call had record_events=False")
        eng = self.engine
        reps = np.arange(self.R, dtype=np.int64) if replicates is None else np.ascontiguousarray(replicates, dtype=np.int64).ravel()
        n = len(reps)
        if n and (reps.min() < 0 or reps.max() >= self.R):
            raise ValueError("replicate index out of range")
        if len(np.unique(reps)) != n:
            raise ValueError("replicates must be distinct")
        counters = [eng.counters(int(r)) for r in reps]
        for r, c in zip(reps, counters):
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        rng = self._walk_starts(reps, counters, seed)
        ts = TreeShapes()
        ts.replicates = reps.copy()
        ts.stats = np.zeros((max(n, 1), len(TreeShapes.STATS)), dtype=np.int64)
        ts.lengths = np.zeros((max(n, 1), len(TreeShapes.LENGTHS)), dtype=np.float64)
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg")}
        rng_out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        io = _capi.VgxTreeShapesIO()
        io.n, io.replicates, io.rng_state = n, _capi._p(reps), rng.ctypes.data_as(u64)
        io.stats, io.lengths = _capi._p(ts.stats), _capi._p(ts.lengths)
        io.status, io.status_arg, io.rng_out = _capi._p(per["status"]), _capi._p(per["status_arg"]), rng_out.ctypes.data_as(u64)
        eng._check(eng.lib.vgx_get_tree_shapes(eng.handle, C.byref(io)))
        ts.stats, ts.lengths = ts.stats[:n], ts.lengths[:n]
        ts.status, ts.status_arg = per["status"][:n], per["status_arg"][:n]
        ts.rng_raw = np.zeros((n, 6), dtype=np.uint64)
        ts.rng_raw[:, :4] = rng_out[:n]
        ts.passes, ts.kernel_ms, ts.clock_ms, ts.wall_ms = int(io.passes), (io.ms[0], io.ms[1]), io.ms[2], io.ms[3]
        return ts

    def tau_tree_shapes(self, seed=None, replicates=None):
        """``tree_shapes()`` for the replicates of the last ``simulate_tau(record_events=True)`` call (``vgx_get_tau_tree_shapes``):
        the walk of ``tau_genealogies(seed, replicates)`` over the same chain with the same draws, status and six generator words
        afterwards, then a kernel that turns every node's event index into its time and the shape kernel of ``tree_shapes()``, all on
        the device: a tau chain needs no host clock, and nothing of a tree crosses to the host.  Returns a :class:`TreeShapes` whose
        rows are what the tree of ``tau_genealogies(seed).replicate(r)`` gives.  A node's time is its prefix event's time or its
        step's: all rows of a step share the step's time, so coalescences inside one step give branches of length 0.

        ``seed`` and ``replicates`` as ``tau_genealogies()`` (``seed=None`` starts every walk at ``(seeds[r], attempt 0, 0 draws)``).
        A replicate whose walk fails (fewer than two samples, a step of more than 8192 raw rows, ...) gets its status, zeros and NaN
        and does not fail the call.  ``kernel_ms``: (canonicalise + walk, node times + shape); ``stage_ms``: the four kernels apart;
        ``clock_ms``: the host's descriptors and step-time tables."""
        self._check_tau_genealogy_call("tau_tree_shapes()")
        eng, lib = self.engine, self.engine.lib
        reps = self._selected_replicates(replicates)
        n = len(reps)
        if seed is not None and not np.isscalar(seed):
            seeds = np.ascontiguousarray(seed, dtype=np.int64).ravel()
            if len(seeds) != n:
                raise ValueError("one seed per selected replicate: got %d for %d" % (len(seeds), n))
        rng = np.zeros((max(n, 1), 6), dtype=np.uint64)
        pos = (C.c_uint64 * 4)()
        for i, r in enumerate(reps):
            lib.vgx_rng_position(int(self.seeds[r]) if seed is None else int(seed) if np.isscalar(seed) else int(seeds[i]), 0, 0, C.byref(pos))
            rng[i, :4] = list(pos)
        pre = self._tau_genealogy_prefix_struct()
        ts = TreeShapes()
        ts.replicates = reps.copy()
        ts.stats = np.zeros((max(n, 1), len(TreeShapes.STATS)), dtype=np.int64)
        ts.lengths = np.zeros((max(n, 1), len(TreeShapes.LENGTHS)), dtype=np.float64)
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg")}
        rng_out = np.zeros((max(n, 1), 6), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        io = _capi.VgxTauTreeShapesIO()
        io.n, io.replicates, io.rng_state = n, _capi._p(reps), rng.ctypes.data_as(u64)
        io.stats, io.lengths = _capi._p(ts.stats), _capi._p(ts.lengths)
        io.status, io.status_arg, io.rng_out = _capi._p(per["status"]), _capi._p(per["status_arg"]), rng_out.ctypes.data_as(u64)
        eng._check(lib.vgx_get_tau_tree_shapes(eng.handle, C.byref(io), C.byref(pre)))
        ts.stats, ts.lengths = ts.stats[:n], ts.lengths[:n]
        ts.status, ts.status_arg = per["status"][:n], per["status_arg"][:n]
        ts.rng_raw = rng_out[:n]
        ts.stage_ms = tuple(io.kernel_ms)
        ts.passes, ts.kernel_ms = int(io.passes), (io.kernel_ms[0] + io.kernel_ms[1], io.kernel_ms[2] + io.kernel_ms[3])
        ts.clock_ms, ts.wall_ms = io.ms[1], io.ms[2]
        return ts

    def _spectrum_blocks(self, io, n, reps, rng, words):
        """The output blocks of a MutationSpectrum behind ``io`` (either of the two io structs); returns (ms, per, rng_out)."""
        S = int(self.engine.dims.sites)
        ms = MutationSpectrum()
        ms.replicates, ms.sites = reps.copy(), S
        ms.spectrum = np.zeros((max(n, 1), S, MutationSpectrum.BINS), dtype=np.int64)
        ms.substitutions = np.zeros((max(n, 1), S, 4, 4), dtype=np.int64)
        ms.sums = np.zeros((max(n, 1), S, len(MutationSpectrum.SUMS)), dtype=np.int64)
        ms.stats = np.zeros((max(n, 1), len(MutationSpectrum.STATS)), dtype=np.int64)
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg")}
        rng_out = np.zeros((max(n, 1), words), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        io.n, io.replicates, io.rng_state = n, _capi._p(reps), rng.ctypes.data_as(u64)
        io.spectrum, io.substitutions, io.sums, io.stats = _capi._p(ms.spectrum), _capi._p(ms.substitutions), _capi._p(ms.sums), _capi._p(ms.stats)
        io.status, io.status_arg, io.rng_out = _capi._p(per["status"]), _capi._p(per["status_arg"]), rng_out.ctypes.data_as(u64)
        return ms, per, rng_out

    def mutation_spectrum(self, seed=None, replicates=None):
        """The site-frequency spectrum of the mutation records of every selected replicate of the last direct
        ``simulate(record_events=True)`` call, on the device (``vgx_get_mutation_spectrum``): the walk of
        ``genealogies(seed, replicates)`` with the same draws, status and generator afterwards, then one kernel that counts the tips
        below every node and bins every mutation record by the clade below its branch.  No node time is needed, so no host clock
        runs: only the rows cross to the host.  Returns a :class:`MutationSpectrum`, whose rows are what the ``tree`` and ``mut_*`` of
        ``genealogies(seed).replicate(r)`` give.

        ``seed`` and ``replicates`` as ``genealogies()``.  A replicate whose walk fails (fewer than two samples, lineages that never
        coalesce, ...) gets its status and zeros and does not fail the call.  Direct chains only."""
        if self._last_call is None:
            raise ValueError("mutation_spectrum() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("mutation_spectrum() walks direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("mutation_spectrum() needs the event log: the last call had record_events=False")
        eng = self.engine
        reps = np.arange(self.R, dtype=np.int64) if replicates is None else np.ascontiguousarray(replicates, dtype=np.int64).ravel()
        n = len(reps)
        if n and (reps.min() < 0 or reps.max() >= self.R):
            raise ValueError("replicate index out of range")
        if len(np.unique(reps)) != n:
            raise ValueError("replicates must be distinct")
        counters = [eng.counters(int(r)) for r in reps]
        for r, c in zip(reps, counters):
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        rng = self._walk_starts(reps, counters, seed)
        io = _capi.VgxMutationSpectrumIO()
        ms, per, rng_out = self._spectrum_blocks(io, n, reps, rng, 4)
        eng._check(eng.lib.vgx_get_mutation_spectrum(eng.handle, C.byref(io)))
        ms.spectrum, ms.substitutions, ms.sums, ms.stats = ms.spectrum[:n], ms.substitutions[:n], ms.sums[:n], ms.stats[:n]
        ms.status, ms.status_arg = per["status"][:n], per["status_arg"][:n]
        ms.rng_raw = np.zeros((n, 6), dtype=np.uint64)
        ms.rng_raw[:, :4] = rng_out[:n]
        ms.passes, ms.kernel_ms, ms.wall_ms = int(io.passes), (io.ms[0], io.ms[1]), io.ms[2]
        return ms

    def tau_mutation_spectrum(self, seed=None, replicates=None):
        """``mutation_spectrum()`` for the replicates of the last ``simulate_tau(record_events=True)`` call
        (``vgx_get_tau_mutation_spectrum``): the walk of ``tau_genealogies(seed, replicates)`` over the same chain with the same
        draws, status and six generator words afterwards, then the spectrum kernel of ``mutation_spectrum()``; nothing of a tree or
        a record crosses to the host.  Returns a :class:`MutationSpectrum` whose rows are what the ``tree`` and ``mut_*`` of
        ``tau_genealogies(seed).replicate(r)`` give.

        ``seed`` and ``replicates`` as ``tau_genealogies()``.  A replicate whose walk fails gets its status and zeros and does not
        fail the call.  ``kernel_ms``: (canonicalise + walk, spectrum); ``stage_ms``: the three kernels apart; ``host_ms``: the
        host's descriptors."""
        self._check_tau_genealogy_call("tau_mutation_spectrum()")
        eng, lib = self.engine, self.engine.lib
        reps = self._selected_replicates(replicates)
        n = len(reps)
        if seed is not None and not np.isscalar(seed):
            seeds = np.ascontiguousarray(seed, dtype=np.int64).ravel()
            if len(seeds) != n:
                raise ValueError("one seed per selected replicate: got %d for %d" % (len(seeds), n))
        rng = np.zeros((max(n, 1), 6), dtype=np.uint64)
        pos = (C.c_uint64 * 4)()
        for i, r in enumerate(reps):
            lib.vgx_rng_position(int(self.seeds[r]) if seed is None else int(seed) if np.isscalar(seed) else int(seeds[i]), 0, 0, C.byref(pos))
            rng[i, :4] = list(pos)
        pre = self._tau_genealogy_prefix_struct()
        io = _capi.VgxTauMutationSpectrumIO()
        ms, per, rng_out = self._spectrum_blocks(io, n, reps, rng, 6)
        eng._check(lib.vgx_get_tau_mutation_spectrum(eng.handle, C.byref(io), C.byref(pre)))
        ms.spectrum, ms.substitutions, ms.sums, ms.stats = ms.spectrum[:n], ms.substitutions[:n], ms.sums[:n], ms.stats[:n]
        ms.status, ms.status_arg = per["status"][:n], per["status_arg"][:n]
        ms.rng_raw = rng_out[:n]
        ms.stage_ms = tuple(io.kernel_ms)
        ms.passes, ms.kernel_ms = int(io.passes), (io.kernel_ms[0] + io.kernel_ms[1], io.kernel_ms[2])
        ms.host_ms, ms.wall_ms = io.ms[1], io.ms[2]
        return ms

    def _introduction_blocks(self, io, n, reps, rng, words):
        """The output blocks of an Introductions behind ``io`` (either of the two io structs); returns (it, per, rng_out)."""
        P = int(self.engine.dims.popNum)
        it = Introductions()
        it.replicates, it.pops = reps.copy(), P
        it.tips_by_pop, it.imports, it.into, it.spectrum, it.stats = _capi._introductions_blocks(max(n, 1), P)
        per = {k: np.zeros(max(n, 1), dtype=np.int64) for k in ("status", "status_arg")}
        rng_out = np.zeros((max(n, 1), words), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        io.n, io.replicates, io.rng_state = n, _capi._p(reps), rng.ctypes.data_as(u64)
        io.tips_by_pop, io.imports, io.into = _capi._p(it.tips_by_pop), _capi._p(it.imports), _capi._p(it.into)
        io.spectrum, io.stats = _capi._p(it.spectrum), _capi._p(it.stats)
        io.status, io.status_arg, io.rng_out = _capi._p(per["status"]), _capi._p(per["status_arg"]), rng_out.ctypes.data_as(u64)
        return it, per, rng_out

    @staticmethod
    def _introduction_rows(it, per, n):
        it.tips_by_pop, it.imports, it.into, it.spectrum, it.stats = it.tips_by_pop[:n], it.imports[:n], it.into[:n], it.spectrum[:n], it.stats[:n]
        it.status, it.status_arg = per["status"][:n], per["status_arg"][:n]

    def introductions(self, seed=None, replicates=None):
        """The transmission lineages of every selected replicate's sampled tree after the last direct
        ``simulate(record_events=True)`` call, on the device (``vgx_get_introductions``): the walk of
        ``genealogies(seed, replicates)`` with the same draws, status and generator afterwards, then one kernel that counts, below
        every node, all tips and the tips reached without a change of population, and bins every branch whose two ends differ in
        population as one net introduction.  No node time is needed, so no host clock runs: only the rows cross to the host.
        Returns an :class:`Introductions`, whose rows are what the ``tree`` and ``tree_pop`` of ``genealogies(seed).replicate(r)``
        give.

        ``seed`` and ``replicates`` as ``genealogies()``.  A replicate whose walk fails (fewer than two samples, lineages that never
        coalesce, ...) gets its status and zeros and does not fail the call.  Direct chains only; at most 1024 populations."""
        if self._last_call is None:
            raise ValueError("introductions() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("introductions() walks direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("introductions() needs the event log: the last call had record_events=False")
        eng = self.engine
        reps = np.arange(self.R, dtype=np.int64) if replicates is None else np.ascontiguousarray(replicates, dtype=np.int64).ravel()
        n = len(reps)
        if n and (reps.min() < 0 or reps.max() >= self.R):
            raise ValueError("replicate index out of range")
        if len(np.unique(reps)) != n:
            raise ValueError("replicates must be distinct")
        counters = [eng.counters(int(r)) for r in reps]
        for r, c in zip(reps, counters):
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        rng = self._walk_starts(reps, counters, seed)
        io = _capi.VgxIntroductionsIO()
        it, per, rng_out = self._introduction_blocks(io, n, reps, rng, 4)
        eng._check(eng.lib.vgx_get_introductions(eng.handle, C.byref(io)))
        self._introduction_rows(it, per, n)
        it.rng_raw = np.zeros((n, 6), dtype=np.uint64)
        it.rng_raw[:, :4] = rng_out[:n]
        it.passes, it.kernel_ms, it.wall_ms = int(io.passes), (io.ms[0], io.ms[1]), io.ms[2]
        return it

    def tau_introductions(self, seed=None, replicates=None):
        """``introductions()`` for the replicates of the last ``simulate_tau(record_events=True)`` call
        (``vgx_get_tau_introductions``): the walk of ``tau_genealogies(seed, replicates)`` over the same chain with the same draws,
        status and six generator words afterwards, then the lineage kernel of ``introductions()``; nothing of a tree or a label
        crosses to the host.  Returns an :class:`Introductions` whose rows are what the ``tree`` and ``tree_pop`` of
        ``tau_genealogies(seed).replicate(r)`` give.

        ``seed`` and ``replicates`` as ``tau_genealogies()``.  A replicate whose walk fails gets its status and zeros and does not
        fail the call.  ``kernel_ms``: (canonicalise + walk, lineages); ``stage_ms``: the three kernels apart; ``host_ms``: the
        host's descriptors."""
        self._check_tau_genealogy_call("tau_introductions()")
        eng, lib = self.engine, self.engine.lib
        reps = self._selected_replicates(replicates)
        n = len(reps)
        if seed is not None and not np.isscalar(seed):
            seeds = np.ascontiguousarray(seed, dtype=np.int64).ravel()
            if len(seeds) != n:
                raise ValueError("one seed per selected replicate: got %d for %d" % (len(seeds), n))
        rng = np.zeros((max(n, 1), 6), dtype=np.uint64)
        pos = (C.c_uint64 * 4)()
        for i, r in enumerate(reps):
            lib.vgx_rng_position(int(self.seeds[r]) if seed is None else int(seed) if np.isscalar(seed) else int(seeds[i]), 0, 0, C.byref(pos))
            rng[i, :4] = list(pos)
        pre = self._tau_genealogy_prefix_struct()
        io = _capi.VgxTauIntroductionsIO()
        it, per, rng_out = self._introduction_blocks(io, n, reps, rng, 6)
        eng._check(lib.vgx_get_tau_introductions(eng.handle, C.byref(io), C.byref(pre)))
        self._introduction_rows(it, per, n)
        it.rng_raw = rng_out[:n]
        it.stage_ms = tuple(io.kernel_ms)
        it.passes, it.kernel_ms = int(io.passes), (io.kernel_ms[0] + io.kernel_ms[1], io.kernel_ms[2])
        it.host_ms, it.wall_ms = io.ms[1], io.ms[2]
        return it

    def milestones(self, variants=None, thresholds=(), replicates=None):
        """Peaks, first passages and extinctions of every selected replicate of the last direct ``simulate(record_events=True)``
        call, per population, over all populations and per variant class, exact over every event and on the device
        (``vgx_get_milestones``): one pass gives every tile of a chain its start values, an ordered walk of the log where the
        kernel left it keeps the running maximum, the first event at or above every threshold and the last event with a host, and
        the tiles are merged with integer atomics.  Returns a :class:`Milestones`.

        ``variants``: as ``prevalence()`` takes them.  ``thresholds``: up to 16 integers in int32 (host counts; any sign).
        ``replicates``: indices (default all, in order).  Direct chains only."""
        if self._last_call is None:
            raise ValueError("milestones() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("milestones() walks direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("milestones() needs the event log: the last call had record_events=False")
        reps = self._selected_replicates(replicates)
        vo, V = _capi.variant_map(variants, self.model.hapNum)
        th = _capi.milestone_thresholds(thresholds)
        n, K, P = len(reps), len(th), self.model.popNum
        _capi.milestones_lds_check(P, V, K)
        eng = self.engine
        for r in reps:
            c = eng.counters(int(r))
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        ms = Milestones()
        ints = {k: np.zeros((n, P + 1, V), dtype=np.int32) for k in ("final", "peak", "peak_event", "last_positive_event")}
        ms.first_event = np.full((n, K, P + 1, V), Milestones.NEVER, dtype=np.int32)
        ms.peak_time, ext_time = np.full((n, P + 1, V), np.nan), np.full((n, P + 1, V), np.nan)
        ms.first_time = np.full((n, K, P + 1, V), np.nan)
        i32 = C.POINTER(C.c_int32)
        io = _capi.VgxMilestonesIO()
        io.n, io.replicates, io.V, io.variant_of, io.K = n, _capi._p(reps), V, vo.ctypes.data_as(i32), K
        io.thresholds = th.ctypes.data_as(i32) if K else None
        if n:
            for k, a in ints.items():
                setattr(io, k, a.ctypes.data_as(i32))
            io.first_event = ms.first_event.ctypes.data_as(i32) if K else None
            io.peak_time, io.extinction_time = _capi._p(ms.peak_time), _capi._p(ext_time)
            io.first_time = _capi._p(ms.first_time) if K else None
        eng._check(eng.lib.vgx_get_milestones(eng.handle, C.byref(io)))
        ms.final, ms.peak, ms.peak_event, ms.last_positive_event = (ints[k] for k in ("final", "peak", "peak_event", "last_positive_event"))
        ms.extinction_time = ext_time
        ms.reached = ms.first_event != Milestones.NEVER
        ms.thresholds, ms.variant_of, ms.replicates = th, vo, reps
        ms._R, ms._scenario_of = self.R, self.scenario_of
        ms._n_scenarios = len(self.scenarios) if self.scenarios is not None else 1
        ms.passes, ms.kernel_ms, ms.clock_ms, ms.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return ms

    def tau_milestones(self, variants=None, thresholds=(), replicates=None):
        """``milestones()`` for the replicates of the last ``simulate_tau(record_events=True)`` call (``vgx_get_tau_milestones``):
        the same arguments and :class:`Milestones`, with ``final`` and ``peak`` int64 and ``thresholds`` up to 16 integers in int64.

        A replicate's chain is ``tau_prevalence()``'s: the model's chain before the tau call (a replicate that restarted has none),
        then its own steps.  An event is a direct event of that earlier chain or one whole step, numbered from 0 along the chain;
        a value is taken after ALL rows of a step, so a step that adds hosts to a cell and takes as many away meets no threshold
        and moves no peak, and a cell whose last host is replaced within a step is not extinct.  The values start as
        ``tau_prevalence()``'s do; event -1 has the time 0.0 for a chain that starts at the beginning of the model's history,
        else the time the call started from.  The shared earlier chain is walked once per call on the device."""
        if self._last_call is None:
            raise ValueError("tau_milestones() needs a simulate_tau(record_events=True) call first")
        if self._last_call[0] != 'tau':
            raise ValueError("tau_milestones() walks tau chains only: the last call was a direct simulate()")
        if not self._last_call[1]:
            raise ValueError("tau_milestones() needs the multievent rows: the last call had record_events=False")
        reps = self._selected_replicates(replicates)
        vo, V = _capi.variant_map(variants, self.model.hapNum)
        th = _capi.tau_milestone_thresholds(thresholds)
        n, K, P = len(reps), len(th), self.model.popNum
        _capi.tau_milestones_lds_check(P, V, K)
        ms = Milestones()
        ms.final, ms.peak = np.zeros((n, P + 1, V), dtype=np.int64), np.zeros((n, P + 1, V), dtype=np.int64)
        ms.peak_event, ms.last_positive_event = np.zeros((n, P + 1, V), dtype=np.int32), np.zeros((n, P + 1, V), dtype=np.int32)
        ms.first_event = np.full((n, K, P + 1, V), Milestones.NEVER, dtype=np.int32)
        ms.peak_time, ms.extinction_time = np.full((n, P + 1, V), np.nan), np.full((n, P + 1, V), np.nan)
        ms.first_time = np.full((n, K, P + 1, V), np.nan)
        i32 = C.POINTER(C.c_int32)
        io = _capi.VgxTauMilestonesIO()
        io.n, io.replicates, io.V, io.variant_of, io.K = n, _capi._p(reps), V, vo.ctypes.data_as(i32), K
        io.thresholds = _capi._p(th) if K else None
        if n:
            io.final, io.peak = _capi._p(ms.final), _capi._p(ms.peak)
            io.peak_event, io.last_positive_event = ms.peak_event.ctypes.data_as(i32), ms.last_positive_event.ctypes.data_as(i32)
            io.first_event = ms.first_event.ctypes.data_as(i32) if K else None
            io.peak_time, io.extinction_time = _capi._p(ms.peak_time), _capi._p(ms.extinction_time)
            io.first_time = _capi._p(ms.first_time) if K else None
        eng, pre = self.engine, self._tau_prefix_struct()
        eng._check(eng.lib.vgx_get_tau_milestones(eng.handle, C.byref(io), C.byref(pre)))
        ms.reached = ms.first_event != Milestones.NEVER
        ms.thresholds, ms.variant_of, ms.replicates = th, vo, reps
        ms._R, (ms._scenario_of, ms._n_scenarios) = self.R, self._scenario_groups()
        ms.passes, ms.kernel_ms, ms.clock_ms, ms.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return ms

    def _prevalence_request(self, g, variants, replicates, summary, values, cell_bytes, scenario_of, n_scenarios, leave_out=None):
        """What ``prevalence()`` and ``tau_prevalence()`` share: the checks on ``replicates``, ``variants``, the LDS limit (cells of
        ``cell_bytes`` bytes), ``summary`` and ``values`` (ValueError before the library is called).  Returns (replicates, n,
        variant_of, V, T, P, the summary's io, its finish)."""
        return self._class_block_request(g, _capi.variant_map, variants, self.model.hapNum, replicates, summary, values, cell_bytes,
                                         scenario_of, n_scenarios, leave_out)

    def _class_block_request(self, g, class_map, classes, members, replicates, summary, values, cell_bytes, scenario_of, n_scenarios,
                             leave_out=None):
        """The request checks of the calls that return a [n, T, P, classes] block (``prevalence``, ``susceptibles`` and their tau
        forms): ``class_map(classes, members)`` is ``_capi.variant_map`` over the haplotypes or ``_capi.group_map`` over the
        susceptibility groups."""
        reps = self._selected_replicates(replicates)
        vo, V = class_map(classes, members)
        T, P = len(g), self.model.popNum
        if cell_bytes * P * V > 65536:
            raise ValueError("%d populations x %d classes need %d bytes of cells, above the 65536 bytes of LDS a counting workgroup may use"
                             % (P, V, cell_bytes * P * V))
        sio, done = self._block_summary(summary, reps, (T, P, V), scenario_of, n_scenarios, leave_out)
        if summary is None and not values:
            raise ValueError("values=False needs summary=: the call would return nothing")
        return reps, len(reps), vo, V, T, P, sio, done

    def susceptibles(self, times=None, points=None, window=None, groups=None, replicates=None, summary=None, values=True):
        """Susceptible hosts per grid time, population and class of susceptibility (immunity) groups of every selected replicate
        of the last direct ``simulate(record_events=True)`` call, on ONE grid for all replicates and on the device
        (``vgx_get_susceptibles``): the other half of the state ``prevalence()`` counts, by the same pass over every replicate's
        log where the kernel left it.  Returns a :class:`Susceptibles`.

        The grid arguments, ``replicates``, ``summary`` and ``values`` are ``prevalence()``'s.  ``groups``: None (every
        susceptibility group its own class), an integer array [susNum] of classes with -1 for groups that are not tracked, or a
        sequence of sequences of group indices (class k = the k-th sequence, the rest not tracked).  With every group tracked
        here and every haplotype tracked in ``prevalence()`` on the same grid, the two blocks add up to the population sizes at
        every grid time.  Direct chains only."""
        g = _prevalence_grid(times, points, window)
        if self._last_call is None:
            raise ValueError("susceptibles() needs a direct simulate(record_events=True) call first")
        if self._last_call[0] != 'direct':
            raise ValueError("susceptibles() counts direct chains only: the last call was simulate_tau")
        if not self._last_call[1]:
            raise ValueError("susceptibles() needs the event log: the last call had record_events=False")
        eng = self.engine
        reps, n, co, G, T, P, sio, done = self._class_block_request(g, _capi.group_map, groups, self.model.susNum, replicates, summary, values, 4,
                                                                    self.scenario_of, len(self.scenarios) if self.scenarios is not None else 1)
        for r in reps:
            c = eng.counters(int(r))
            if c.ev_first_new != 0:
                raise ValueError("replicate %d: its chain does not start in the last call's device log (the model held %d events "
                                 "when the ensemble started)" % (r, c.ev_first_new))
        block = np.zeros((n, T, P, G), dtype=np.int32) if values else None
        final = np.zeros((n, P, G), dtype=np.int32)
        outside = np.zeros((max(n, 1), 2), dtype=np.int64)
        i32 = C.POINTER(C.c_int32)
        io = _capi.VgxSusceptiblesIO()
        io.n, io.replicates, io.T, io.grid, io.G, io.class_of = n, _capi._p(reps), T, _capi._p(g), G, co.ctypes.data_as(i32)
        io.values = block.ctypes.data_as(i32) if values and n else None
        io.final = final.ctypes.data_as(i32) if n else None
        io.outside = _capi._p(outside)
        io.summary = C.pointer(sio) if sio is not None and n else None
        eng._check(eng.lib.vgx_get_susceptibles(eng.handle, C.byref(io)))
        return Susceptibles._of(block, final, g, co, outside[:n], reps, done, io)

    def tau_susceptibles(self, times=None, points=None, window=None, groups=None, replicates=None, summary=None, values=True):
        """``susceptibles()`` for the replicates of the last ``simulate_tau(record_events=True)`` call
        (``vgx_get_tau_susceptibles``): the same arguments and :class:`Susceptibles`, with ``values`` [n, T, P, G] and ``final``
        [n, P, G] int64 and ``outside`` the summed multiplicities, as ``tau_prevalence()`` has them.  The chain, the time of a
        step, the start state (the model's initial susceptible state when the chain starts at the beginning of the model's
        history, else the state the call started from) and the summary's refusals are ``tau_prevalence()``'s."""
        g = _prevalence_grid(times, points, window)
        if self._last_call is None:
            raise ValueError("tau_susceptibles() needs a simulate_tau(record_events=True) call first")
        if self._last_call[0] != 'tau':
            raise ValueError("tau_susceptibles() counts tau chains only: the last call was a direct simulate()")
        if not self._last_call[1]:
            raise ValueError("tau_susceptibles() needs the multievent rows: the last call had record_events=False")
        reps, n, co, G, T, P, sio, done = self._class_block_request(g, _capi.group_map, groups, self.model.susNum, replicates, summary, values, 8,
                                                                    *self._scenario_groups())
        block = np.zeros((n, T, P, G), dtype=np.int64) if values else None
        final = np.zeros((n, P, G), dtype=np.int64)
        outside = np.zeros((max(n, 1), 2), dtype=np.int64)
        io = _capi.VgxTauSusceptiblesIO()
        io.n, io.replicates, io.T, io.grid, io.G = n, _capi._p(reps), T, _capi._p(g), G
        io.class_of = co.ctypes.data_as(C.POINTER(C.c_int32))
        io.values = _capi._p(block) if values and n else None
        io.final = _capi._p(final) if n else None
        io.outside = _capi._p(outside)
        io.summary = C.pointer(sio) if sio is not None and n else None
        eng, pre = self.engine, self._tau_prefix_struct()
        eng._check(eng.lib.vgx_get_tau_susceptibles(eng.handle, C.byref(io), C.byref(pre)))
        return Susceptibles._of(block, final, g, co, outside[:n], reps, done, io)

    def tau_prevalence(self, times=None, points=None, window=None, variants=None, replicates=None, summary=None, values=True):
        """``prevalence()`` for the replicates of the last ``simulate_tau(record_events=True)`` call (``vgx_get_tau_prevalence``):
        the same grid arguments, ``variants``, ``summary`` and :class:`Prevalence`, with ``values`` [n, T, P, V] and ``final``
        [n, P, V] int64 (an interval sums the multiplicities of many steps) and ``outside`` the summed multiplicities up to
        ``times[0]`` and after ``times[T - 1]``.

        A replicate's chain is the model's chain before the tau call (a replicate that restarted has none), then its own steps,
        every multievent row changing its cells by ``num``.  All events of a step carry the time of the step's MULTITYPE record, so
        a grid time at exactly a step's time has the whole step applied, as ``simulate_tau(traj_points=, traj_window=)`` has.  The
        values start from the model's initial state when the chain starts at the beginning of the model's history (the model held
        events before the call, or the replicate restarted), else from the state the call started from.  The shared part is
        counted once per call on the device, not once per replicate; no host clock runs.  ``summary``: refused by the library
        when a value is negative or reaches 2^31 (``values`` stays available: call again without ``summary``).  ``by='auto'``:
        one group per scenario of a scenario ensemble."""
        g = _prevalence_grid(times, points, window)
        if self._last_call is None:
            raise ValueError("tau_prevalence() needs a simulate_tau(record_events=True) call first")
        if self._last_call[0] != 'tau':
            raise ValueError("tau_prevalence() counts tau chains only: the last call was a direct simulate()")
        if not self._last_call[1]:
            raise ValueError("tau_prevalence() needs the multievent rows: the last call had record_events=False")
        reps, n, vo, V, T, P, sio, done = self._prevalence_request(g, variants, replicates, summary, values, 8, *self._scenario_groups())
        block = np.zeros((n, T, P, V), dtype=np.int64) if values else None
        final = np.zeros((n, P, V), dtype=np.int64)
        outside = np.zeros((max(n, 1), 2), dtype=np.int64)
        io = _capi.VgxTauPrevalenceIO()
        io.n, io.replicates, io.T, io.grid, io.V = n, _capi._p(reps), T, _capi._p(g), V
        io.variant_of = vo.ctypes.data_as(C.POINTER(C.c_int32))
        io.values = _capi._p(block) if values and n else None
        io.final = _capi._p(final) if n else None
        io.outside = _capi._p(outside)
        io.summary = C.pointer(sio) if sio is not None and n else None
        eng, pre = self.engine, self._tau_prefix_struct()
        eng._check(eng.lib.vgx_get_tau_prevalence(eng.handle, C.byref(io), C.byref(pre)))
        pv = Prevalence()
        pv.values, pv.final, pv.times, pv.variant_of, pv.outside, pv.replicates = block, final, g, vo, outside[:n], reps
        pv.summary = done() if done is not None else None
        pv.passes, pv.kernel_ms, pv.clock_ms, pv.wall_ms = int(io.passes), io.ms[0], io.ms[1], io.ms[2]
        return pv

    def trajectories(self, out=None):
        """Summary trajectories of the last call, ``[R, T, P, 2]`` float64 (infectious, susceptible per population).
        ``out`` may be a CUDA torch tensor (filled on the device, no host round trip) or None (numpy)."""
        if self.traj_shape is None:
            raise RuntimeError("the last simulate() call did not record trajectories (traj_points=0)")
        eng = self.engine
        if out is None:
            a = np.empty(self.traj_shape, dtype=np.float64)
            eng._check(eng.lib.vgx_get_trajectories(eng.handle, a.ctypes.data_as(C.c_void_p), 0))
            return a
        assert tuple(out.shape) == self.traj_shape and out.is_contiguous() and str(out.dtype) == "torch.float64"
        eng._check(eng.lib.vgx_get_trajectories(eng.handle, C.c_void_p(out.data_ptr()), 1 if out.is_cuda else 0))
        return out

    def trajectory_summary(self, quantiles=(0.025, 0.5, 0.975), by='auto', replicates=None, method='linear'):
        """Bands of the last call's trajectories across replicates, formed on the device (``vgx_get_trajectory_summary``; the
        ``[R, T, P, 2]`` block is not copied to the host): count, mean, variance, min, max and quantiles per group, time point,
        population and compartment.  Returns a :class:`TrajectorySummary`.

        ``by``: 'auto' = one group per scenario of a scenario ensemble, else one group of all replicates; or an integer array
        ``[R]`` of group labels in [0, R) (groups 0 .. max label; a label nobody carries is an empty group).  ``replicates``: indices
        (or a boolean mask) of the replicates that take part; the others are left out of every group.  ``method``: 'lower' /
        'higher' give the member value at rank floor / ceil of q (m - 1) among the group's m values (exact; numpy's methods of
        the same names); 'linear' (numpy's default) asks the device for both neighbours and interpolates on the host: with
        i = q (m - 1), t = i - floor(i): ``v[floor(i)] + (v[floor(i) + 1] - v[floor(i)]) t``.  A group of more than 16 384
        members is refused by the library."""
        if self.traj_shape is None:
            raise ValueError("trajectory_summary() needs trajectories: the last simulate call recorded none (traj_points=0)")
        q = _summary_quantiles(quantiles, method)
        R, T, P, _ = self.traj_shape
        group_of, G = _summary_groups(by, replicates, R, self.scenario_of, len(self.scenarios) if self.scenarios is not None else 1)
        io, finish = _summary_request(group_of, G, q, method, (T, P, 2))
        eng = self.engine
        eng._check(eng.lib.vgx_get_trajectory_summary(eng.handle, C.byref(io)))
        return finish()

    def gather_trajectories(self, dst=0, out=None, async_op=False, wire_dtype=None, device=None):
        """One collective for the whole ensemble: every rank's ``[R, T, P, 2]`` block to rank ``dst``
        (``torch.distributed.gather``; backend nccl = RCCL over xGMI, gloo on CPU).  Returns the stacked
        ``[world, R, T, P, 2]`` tensor on ``dst`` and None elsewhere; ``out`` may be a preallocated result tensor on
        ``dst``.  With ``async_op=True`` the trajectories are first copied out of the engine (so the next ``simulate``
        may overwrite them) and a :class:`PendingGather` is returned: the transfer overlaps the next step and
        ``.wait()`` gives the result.  ``wire_dtype=torch.int32`` sends the compartment totals as 32-bit integers (they are
        whole numbers; refused unless every population size is below 2^31): half the bytes on every xGMI link and in the
        result on ``dst``, which then has that dtype.  Without a process group (one rank) the result is a host tensor, or — with
        ``device='cuda'`` — a tensor on the engine's GPU, filled there: where an RCCL gather leaves it on rank ``dst``."""
        import torch
        import torch.distributed as dist

        def narrow(t):
            if wire_dtype is None or wire_dtype == torch.float64:
                return t
            if wire_dtype != torch.int32:
                raise ValueError("wire_dtype must be None, torch.float64 or torch.int32")
            if int(np.max(self.model.sizes)) >= 2 ** 31:
                raise ValueError("wire_dtype=int32 needs population sizes below 2^31")
            return t.to(torch.int32)

        if not (dist.is_available() and dist.is_initialized()):
            if device is not None and str(device).startswith("cuda"):
                dev = torch.device("cuda", torch.cuda.current_device()) if str(device) == "cuda" else torch.device(device)
                res = narrow(self.trajectories(torch.empty(self.traj_shape, dtype=torch.float64, device=dev)))[None]
            else:
                res = narrow(torch.from_numpy(self.trajectories()))[None]
            return PendingGather(None, res, None) if async_op else res
        backend = dist.get_backend()
        if backend == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
            if wire_dtype == torch.int32:      # narrowed on the device straight from the engine's buffer: no f64 copy
                narrow(torch.empty(0))         # (the checks)
                mine = torch.empty(self.traj_shape, dtype=torch.int32, device=dev)
                eng = self.engine
                eng._check(eng.lib.vgx_get_trajectories_int(eng.handle, C.c_void_p(mine.data_ptr())))
            else:
                mine = narrow(self.trajectories(torch.empty(self.traj_shape, dtype=torch.float64, device=dev)))
        else:
            mine = narrow(torch.from_numpy(self.trajectories()))
        world, rank = dist.get_world_size(), dist.get_rank()
        if rank == dst:   # gather straight into the rows of the result: no second copy of [world, R, T, P, 2]
            if out is None:
                out = torch.empty((world,) + tuple(mine.shape), dtype=mine.dtype, device=mine.device)
            assert tuple(out.shape) == (world,) + tuple(mine.shape) and out.is_contiguous()
            assert out.dtype == mine.dtype and out.device == mine.device, "`out` must have the wire dtype and live where the collective runs"
            work = dist.gather(mine, list(out.unbind(0)), dst=dst, async_op=async_op)
        else:
            out = None
            work = dist.gather(mine, None, dst=dst, async_op=async_op)
        return PendingGather(work, out, mine) if async_op else out


class GenealogyBatch:
    """Genealogies of many replicates (``Ensemble.genealogies``), as flat arrays with per-replicate offsets.

    ``replicates[i]`` is the replicate of row i; ``status[i]`` is 0 or why its walk stopped (``message(i)``).  Nodes of row i
    are ``tree`` / ``tree_pop`` / ``times``[node_offsets[i]:node_offsets[i+1]] (node ids local to the replicate, 0 ..
    2 sCounter - 2), its mutation records ``mut_*``[mut_offsets[i]:mut_offsets[i+1]], its migration records likewise
    ``mig_*``; failed rows hold none.  ``nodes_used[i]``, ``rng_raw[i]`` (the generator after the walk)."""

    NODE_KEYS = ("tree", "tree_pop", "times")
    MUT_KEYS = ("mut_node", "mut_AS", "mut_DS", "mut_site", "mut_time")
    MIG_KEYS = ("mig_node", "mig_time", "mig_old", "mig_new")

    def __init__(self, replicates):
        self.replicates = np.asarray(replicates, dtype=np.int64).copy()
        self._row = {int(r): i for i, r in enumerate(self.replicates)}

    def _fill(self, off, cap, per, rng_out):
        n = len(self.replicates)
        self.status, self.status_arg = per["status"].copy(), per["status_arg"].copy()
        ok = self.status == 0
        self.nodes_used = per["nodes_used"].copy()
        self.rng_raw = np.zeros((n, 6), dtype=np.uint64)
        self.rng_raw[:, :rng_out.shape[1]] = rng_out   # (tau batches: the buffered 32-bit half too)

        def compact(o, keep, keys):   # row i keeps the first keep[i] entries of its capacity
            lens = np.diff(o)
            pos = np.arange(int(o[-1]), dtype=np.int64) - np.repeat(o[:-1], lens)
            mask = pos < np.repeat(keep, lens)
            for k in keys:
                setattr(self, k, cap[k][:len(mask)][mask])
            return np.concatenate(([0], np.cumsum(keep))).astype(np.int64)
        self.node_offsets = compact(off["node"], np.where(ok, np.diff(off["node"]), 0), self.NODE_KEYS)
        self.mut_offsets = compact(off["mut"], np.where(ok, per["mut_n"], 0), self.MUT_KEYS)
        self.mig_offsets = compact(off["mig"], np.where(ok, per["mig_n"], 0), self.MIG_KEYS)

    def __len__(self):
        return len(self.replicates)

    def message(self, i):
        """Text of row i's status: what ``Ensemble.genealogy`` raises for that replicate ('' when it succeeded)."""
        return _capi.genealogy_message(int(self.status[i]), int(self.status_arg[i]))

    def replicate(self, r):
        """The genealogy of replicate ``r`` as ``Ensemble.genealogy(r, seed_r)`` returns it; raises what that raises when
        the walk of ``r`` failed."""
        i = self._row.get(int(r))
        if i is None:
            raise KeyError("replicate %d is not in this batch" % r)
        if self.status[i] != 0:
            raise RuntimeError(self.message(i))
        out = {}
        for keys, o in ((self.NODE_KEYS, self.node_offsets), (self.MUT_KEYS, self.mut_offsets), (self.MIG_KEYS, self.mig_offsets)):
            for k in keys:
                out[k] = getattr(self, k)[o[i]:o[i + 1]].copy()
        out["nodes_used"] = int(self.nodes_used[i])
        out["rng_raw"] = tuple(int(x) for x in self.rng_raw[i])
        return out


class TimelineBatch:
    """Compartment series of many replicates (``Ensemble.timelines``) as flat arrays; T = step_num + 1.

    ``replicates[i]`` is the replicate of row i; ``time_points[i]`` its grid (``k * currentTime / step_num`` of its own final
    time); ``infectious[i, k]`` / ``samples[i, k]`` the ``Data`` / ``Sample`` series of ``infectious_queries[k]`` = (population,
    haplotype); ``susceptible[i, k]`` the series of ``susceptible_queries[k]`` = (population, group); ``last_point[i]`` the last
    grid index the replay reached.  All series are float64 whole numbers."""

    def __init__(self, replicates, infectious_queries, susceptible_queries, step_num, semantics):
        self.replicates = np.asarray(replicates, dtype=np.int64).copy()
        self._row = {int(r): i for i, r in enumerate(self.replicates)}
        self.infectious_queries = np.asarray(infectious_queries, dtype=np.int64).reshape(-1, 2)
        self.susceptible_queries = np.asarray(susceptible_queries, dtype=np.int64).reshape(-1, 2)
        self.step_num, self.semantics = int(step_num), semantics

    def __len__(self):
        return len(self.replicates)

    def _index(self, r):
        i = self._row.get(int(r))
        if i is None:
            raise KeyError("replicate %d is not in this batch" % r)
        return i

    def lockdowns(self, r, pop):
        """``[[state, time], ...]`` of population ``pop`` of replicate ``r`` (times from the host clock)."""
        i = self._index(r)
        n, st, pp, tt = self._loc
        return [[bool(st[i, k]), float(tt[i, k])] for k in range(int(n[i])) if pp[i, k] == pop]

    def data_infectious(self, r, k):
        """``(Data, Sample, time_points, lockdowns)`` as ``BirthDeathModel.get_data_infectious(pop, hap, step_num)`` returns
        them for replicate ``r`` and infectious query ``k``."""
        i = self._index(r)
        return (self.infectious[i, k].copy(), self.samples[i, k].copy(), [float(t) for t in self.time_points[i]],
                self.lockdowns(r, int(self.infectious_queries[k, 0])))

    def data_susceptible(self, r, k):
        """``(Data, time_points, lockdowns)`` as ``BirthDeathModel.get_data_susceptible(pop, group, step_num)`` returns them."""
        i = self._index(r)
        return (self.susceptible[i, k].copy(), [float(t) for t in self.time_points[i]],
                self.lockdowns(r, int(self.susceptible_queries[k, 0])))


class PendingGather:
    """Handle of an asynchronous trajectory gather: keeps the send/receive buffers alive until ``wait()``."""

    def __init__(self, work, result, keep):
        self.work, self.result, self.keep = work, result, keep

    def wait(self):
        if self.work is not None:
            self.work.wait()
            self.work = None
        self.keep = None
        return self.result
