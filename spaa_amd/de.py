"""SciPy's `differential_evolution` (SciPy 1.15.3, scipy/optimize/_differentialevolution.py) restated in numpy for the
configurations the One-pixel attacker uses (one_pixel_attacker/__init__.py:88-89), with a BATCHED objective.

Supported: strategy 'best1bin', init 'latinhypercube', `mutation` as a float or a dithering (min, max) pair, any
`recombination`, `tol` / `atol`, an old-style `callback(xk, convergence)` whose truthy return stops after the generation,
`polish=False`, `maxiter`, `popsize` (a multiplier of the parameter count), `updating` 'immediate' or 'deferred'.

Randomness comes from numpy in SciPy's draw order: the LHS samples and the per-parameter permutations; the dither draw at the
start of every generation; per trial, the `fill_point` integer, the in-place shuffle of the persistent population-index
permutation (`_select_samples`), the crossover uniforms and the out-of-bounds redraws of `_ensure_constraint`.  `seed=None`
is numpy's global RandomState (what the reference relies on through `reset_rng_seeds(0)`), an int seeds a new RandomState, a
RandomState is used as it is.

`objective(params[S, N]) -> energies[S]`.  With updating='immediate' (SciPy's default, the reference's semantics) the trials of
a generation are evaluated SPECULATIVELY, `max_batch` at a time: each is built as if none before it is accepted.  Walking the
results in order, an accepted trial j changes row j (and rows 0 and l when the best moves); the first later trial that read
a changed row (its own row, row 0, or one of its two difference vectors) is discarded with everything after it, the RNG and
the permutation are restored to their state before it, and speculation restarts there.  The objective values DE consumes,
`x`, `fun`, `nfev`, `nit` and the RNG state afterwards are therefore SciPy's; discarded evaluations do not count in `nfev`
(`evaluated` counts them).  With `max_batch=1` the walk is SciPy's loop.  updating='deferred' evaluates one batch per
generation, as SciPy's deferred mode does.
"""
import numbers

import numpy as np

_MACHEPS = np.finfo(np.float64).eps
_MSG_SUCCESS = 'Optimization terminated successfully.'
_MSG_MAXITER = 'Maximum number of iterations has been exceeded.'
_MSG_CALLBACK = 'callback function requested stop early'


class DEResult(dict):
    """x, fun, nfev, nit, success, message, and `evaluated`: candidates actually evaluated (speculation included)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _check_random_state(seed):
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (numbers.Integral, np.integer)):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f'seed must be None, an int or a numpy RandomState (got {type(seed).__name__})')


class DifferentialEvolution:
    """The solver state (SciPy's DifferentialEvolutionSolver for the supported subset).  `_accept` is the one comparison
    every acceptance decision goes through."""

    def __init__(self, objective, bounds, strategy='best1bin', maxiter=1000, popsize=15, tol=0.01, mutation=(0.5, 1),
                 recombination=0.7, seed=None, callback=None, polish=False, init='latinhypercube', atol=0,
                 updating='immediate', max_batch=None):
        if strategy != 'best1bin':
            raise NotImplementedError(f'strategy {strategy!r}: only best1bin is restated')
        if init != 'latinhypercube':
            raise NotImplementedError(f'init {init!r}: only latinhypercube is restated')
        if polish:
            raise NotImplementedError('polish=True (L-BFGS-B polishing) is not restated: pass polish=False')
        if updating not in ('immediate', 'deferred'):
            raise ValueError(f'updating must be immediate or deferred (got {updating!r})')
        if (not np.all(np.isfinite(mutation)) or np.any(np.array(mutation) >= 2) or np.any(np.array(mutation) < 0)):
            raise ValueError('The mutation constant must be a float in U[0, 2), or specified as a tuple(min, max) where '
                             'min < max and min, max are in U[0, 2).')
        self.objective, self.callback, self.updating = objective, callback, updating
        self.scale = mutation
        self.dither = sorted([mutation[0], mutation[1]]) if hasattr(mutation, '__iter__') and len(mutation) > 1 else None
        self.cr = recombination
        self.tol, self.atol = tol, atol
        self.limits = np.array(bounds, dtype='float').T
        if np.size(self.limits, 0) != 2 or not np.all(np.isfinite(self.limits)):
            raise ValueError('bounds should be a sequence containing finite real valued (min, max) pairs for each value in x')
        self.maxiter = 1000 if maxiter is None else maxiter
        self._arg1 = 0.5 * (self.limits[0] + self.limits[1])
        self._arg2 = np.fabs(self.limits[0] - self.limits[1])
        self.N = np.size(self.limits, 1)
        self.rng = _check_random_state(seed)
        eb_count = np.count_nonzero(self.limits[0] == self.limits[1])
        self.M = max(5, popsize * max(1, self.N - eb_count))
        self.max_batch = self.M if max_batch is None else int(max_batch)
        if self.max_batch < 1:
            raise ValueError('max_batch must be >= 1')
        self.nfev = self.evaluated = 0
        # init_population_lhs
        segsize = 1.0 / self.M
        samples = (segsize * self.rng.uniform(size=(self.M, self.N))
                   + np.linspace(0., 1., self.M, endpoint=False)[:, np.newaxis])
        self.population = np.zeros_like(samples)
        for j in range(self.N):
            order = self.rng.permutation(range(self.M))
            self.population[:, j] = samples[order, j]
        self.energies = np.full(self.M, np.inf)
        self._perm = np.arange(self.M)      # SciPy's persistent _random_population_index
        self.consumed = None                # set to a list: receives (params, energy) of every evaluation DE consumes, in order

    # -- SciPy's helpers -------------------------------------------------------------------------------------------------
    def scale_parameters(self, trial):
        return self._arg1 + (trial - 0.5) * self._arg2

    @property
    def x(self):
        return self.scale_parameters(self.population[0])

    def convergence(self):
        if np.any(np.isinf(self.energies)):
            return np.inf
        return np.std(self.energies) / (np.abs(np.mean(self.energies)) + _MACHEPS)

    def converged(self):
        if np.any(np.isinf(self.energies)):
            return False
        return np.std(self.energies) <= self.atol + self.tol * np.abs(np.mean(self.energies))

    def _accept(self, e_trial, e_orig, trial, orig):
        """SciPy's _accept_trial without constraints; `trial` / `orig` are the two population vectors in [0, 1] (for
        subclasses that audit the comparisons)."""
        return e_trial <= e_orig

    def _consume(self, trials, energies):
        if self.consumed is not None:
            self.consumed.extend(zip(self.scale_parameters(trials), energies))

    def _promote_lowest_energy(self):
        l = int(np.argmin(self.energies))
        self.energies[[0, l]] = self.energies[[l, 0]]
        self.population[[0, l], :] = self.population[[l, 0], :]
        return l

    def _select_samples(self, candidate, number_samples=5):
        self.rng.shuffle(self._perm)
        idxs = self._perm[:number_samples + 1]
        return idxs[idxs != candidate][:number_samples]

    def _ensure_constraint(self, trial):
        mask = np.bitwise_or(trial > 1, trial < 0)
        oob = np.count_nonzero(mask)
        if oob:
            trial[mask] = self.rng.uniform(size=oob)

    def _mutate(self, candidate):
        """One best1bin trial (SciPy's _mutate + _ensure_constraint).  Returns (trial, rows it read)."""
        fill_point = self.rng.randint(self.N, size=None, dtype='int64')
        samples = self._select_samples(candidate, 5)
        trial = np.copy(self.population[candidate])
        r0, r1 = samples[..., :2].T
        bprime = self.population[0] + self.scale * (self.population[r0] - self.population[r1])
        crossovers = self.rng.uniform(size=self.N) < self.cr
        crossovers[fill_point] = True
        trial = np.where(crossovers, bprime, trial)
        self._ensure_constraint(trial)
        return trial, (candidate, 0, int(r0), int(r1))

    def _evaluate(self, trials):
        """Scaled parameters of `trials` [S, N] through the objective, max_batch rows per call."""
        params = self.scale_parameters(trials)
        out = []
        for s in range(0, len(params), self.max_batch):
            e = np.asarray(self.objective(params[s:s + self.max_batch]))
            if e.shape != (min(self.max_batch, len(params) - s),):
                raise RuntimeError(f'objective must return energies of shape (S,) for params of shape (S, N) (got {e.shape})')
            out.append(e)
        self.evaluated += len(params)
        return np.concatenate(out) if out else np.zeros(0)

    # -- one generation --------------------------------------------------------------------------------------------------
    def _generation_immediate(self):
        c = 0
        while c < self.M:
            stop = min(c + self.max_batch, self.M)
            trials, reads, states = [], [], []
            for j in range(c, stop):
                states.append((self.rng.get_state(), self._perm.copy()))
                t, r = self._mutate(j)
                trials.append(t)
                reads.append(r)
            energies = self._evaluate(np.array(trials))
            end = stop             # first trial that is not consumed
            j = c
            while j < end:
                i = j - c
                e = energies[i]
                self.nfev += 1
                self._consume(trials[i][None], energies[i:i + 1])
                if self._accept(e, self.energies[j], trials[i], self.population[j]):
                    self.population[j] = trials[i]
                    self.energies[j] = np.squeeze(e)
                    changed = {j}
                    if self._accept(e, self.energies[0], trials[i], self.population[0]):
                        l = self._promote_lowest_energy()
                        if l != 0:
                            changed.update((0, l))
                    for t in range(j + 1, end):
                        if changed.intersection(reads[t - c]):
                            end = t
                            break
                j += 1
            if end < stop:
                state, perm = states[end - c]
                self.rng.set_state(state)
                self._perm[:] = perm
            c = end

    def _generation_deferred(self):
        cands = np.arange(self.M)
        trial = np.copy(self.population[cands])
        samples = np.array([self._select_samples(c, 5) for c in cands])
        r0, r1 = samples[..., :2].T
        bprime = self.population[0] + self.scale * (self.population[r0] - self.population[r1])
        fill_point = self.rng.randint(self.N, size=self.M, dtype='int64')
        crossovers = self.rng.uniform(size=(self.M, self.N)) < self.cr
        crossovers[cands, fill_point[cands]] = True
        trial = np.where(crossovers, bprime, trial)
        self._ensure_constraint(trial)
        e_trial = self._evaluate(trial)
        self.nfev += self.M
        self._consume(trial, e_trial)
        loc = np.array([self._accept(e_trial[k], self.energies[k], trial[k], self.population[k]) for k in range(self.M)])
        self.population = np.where(loc[:, np.newaxis], trial, self.population)
        self.energies = np.where(loc, e_trial, self.energies)
        self._promote_lowest_energy()

    def solve(self):
        nit, warning_flag, message = 0, False, _MSG_SUCCESS
        if np.all(np.isinf(self.energies)):
            e = self._evaluate(self.population)
            self.energies[:] = e
            self.nfev += self.M
            self._consume(self.population, e)
            self._promote_lowest_energy()
        for nit in range(1, self.maxiter + 1):
            if self.dither is not None:
                self.scale = self.rng.uniform(self.dither[0], self.dither[1])
            if self.updating == 'immediate':
                self._generation_immediate()
            else:
                self._generation_deferred()
            if self.callback is not None:
                c = self.tol / (self.convergence() + _MACHEPS)
                try:
                    warning_flag = bool(self.callback(np.copy(self.x), c))
                except StopIteration:
                    warning_flag = True
                if warning_flag:
                    message = _MSG_CALLBACK
            if warning_flag or self.converged():
                break
        else:
            message, warning_flag = _MSG_MAXITER, True
        return DEResult(x=self.x, fun=self.energies[0], nfev=self.nfev, nit=nit, success=(warning_flag is not True),
                        message=message, evaluated=self.evaluated)


def differential_evolution(objective, bounds, strategy='best1bin', maxiter=1000, popsize=15, tol=0.01, mutation=(0.5, 1),
                           recombination=0.7, seed=None, callback=None, polish=False, init='latinhypercube', atol=0,
                           updating='immediate', max_batch=None):
    """scipy.optimize.differential_evolution (1.15.3) for a batched `objective(params[S, N]) -> energies[S]`; see the module
    docstring.  `max_batch`: trials per objective call (default: the population size).  Returns a DEResult."""
    return DifferentialEvolution(objective, bounds, strategy, maxiter, popsize, tol, mutation, recombination, seed, callback,
                                 polish, init, atol, updating, max_batch).solve()
