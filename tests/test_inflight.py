"""writers.InflightWindow against a literal transcription of the three loops it replaced (main's
batch loop, _run_gpu_workers.drain and ShardWriters.add of the previous pretrain.py): the same
futures are waited for, in the same order, and the same files counted, after every step."""
import random
import threading

from lddl_amd.dask.bert.writers import InflightWindow


class Fut:
    """A finished future that logs its .result() call."""

    def __init__(self, log, tag, value=None, nbytes=None):
        self.log, self.tag, self.value = log, tag, value
        if nbytes is not None:
            self.render_bytes = nbytes

    def result(self):
        self.log.append(self.tag)
        return self.value


class ModelAfterPush:
    """main's loop (limit 2) and _run_gpu_workers.drain (limit n_workers + 1; without the lock,
    which one thread does not need): checked after the append."""

    def __init__(self, limit_batches, limit_bytes):
        self.limit_batches, self.limit_bytes = limit_batches, limit_bytes
        self.inflight, self.n_files = [], 0

    def _wait(self):
        j, fs = self.inflight.pop(0)
        if not isinstance(j, list):
            self.n_files += len(j.result())
        for f in fs:
            f.result()

    def step(self, job, futs):
        if isinstance(job, list):
            self.n_files += len(job)
        self.inflight.append((job, futs))
        while len(self.inflight) > self.limit_batches or (len(self.inflight) > 1 and sum(
                getattr(j, 'render_bytes', 0) for j, _ in self.inflight) > self.limit_bytes):
            self._wait()

    def finish(self):  # main's final loop, _run_gpu_workers' drain(0, 0)
        while self.inflight:
            self._wait()


class ModelBeforePush:
    """ShardWriters.add: checked before the copy job is submitted."""

    def __init__(self, max_inflight_bytes):
        self.max_inflight_bytes, self.jobs = max_inflight_bytes, []

    def step(self, submit, nb, writes):
        while self.jobs and (len(self.jobs) >= 2 or
                             sum(b for _, b, _ in self.jobs) + nb > self.max_inflight_bytes):
            j, _, ws = self.jobs.pop(0)
            j.result()
            for f in ws:
                f.result()
        self.jobs.append((submit(), nb, writes))


def _sizes(rng, n, max_bytes):
    """Zeros (jobs that are lists of paths), sizes around the bound and some above it."""
    top = max(max_bytes, 4)
    return [rng.choice([0, 0, rng.randrange(1, top + 1), rng.randrange(1, top // 2 + 1),
                        top + rng.randrange(1, 100)]) for _ in range(n)]


def _job(log, k, nbytes, rng):
    """Entry k's (job, write futures): a list of paths for 0 bytes, else a copy future."""
    paths = ['p{}.{}'.format(k, i) for i in range(rng.randrange(0, 4))]
    futs = [Fut(log, ('w', k, i)) for i in range(rng.randrange(0, 3))]
    if nbytes == 0:
        return paths, futs
    return Fut(log, ('j', k), paths, nbytes), futs


def test_window_after_push_matches_the_batch_loops():
    rng = random.Random(20)
    for case in range(300):
        max_batches = rng.choice([2, 2, 3, 4, 5])  # main: 2; workers: n_workers + 1
        max_bytes = rng.choice([0, 1, 10, 100, 1000])
        log_m, log_w = [], []
        model = ModelAfterPush(max_batches, max_bytes)
        win = InflightWindow(max_batches, max_bytes)
        for k, nb in enumerate(_sizes(rng, rng.randrange(1, 12), max_bytes)):
            state = rng.getstate()
            job, futs = _job(log_m, k, nb, rng)
            model.step(job, futs)
            rng.setstate(state)
            job, futs = _job(log_w, k, nb, rng)
            win.push(job, futs, getattr(job, 'render_bytes', 0))
            win.trim()
            assert log_w == log_m and win.n_files == model.n_files, (case, k)
            assert len(win) == len(model.inflight)
        model.finish()
        win.drain()
        assert log_w == log_m and win.n_files == model.n_files and len(win) == 0, case


def test_window_trim_incoming_matches_shard_writers_add():
    rng = random.Random(21)
    for case in range(300):
        max_bytes = rng.choice([0, 1, 10, 100, 1000])
        log_m, log_w = [], []
        model = ModelBeforePush(max_bytes)
        win = InflightWindow(2, max_bytes)
        for k, nb in enumerate(_sizes(rng, rng.randrange(1, 12), max_bytes)):
            nw = rng.randrange(0, 3)
            # the copy job is submitted only after the older batches were waited for
            model.step(lambda: log_m.append(('submit', k)) or Fut(log_m, ('j', k)), nb,
                       [Fut(log_m, ('w', k, i)) for i in range(nw)])
            win.trim(incoming=nb)
            log_w.append(('submit', k))
            win.push(Fut(log_w, ('j', k)), [Fut(log_w, ('w', k, i)) for i in range(nw)], nb)
            assert log_w == log_m and len(win) == len(model.jobs), (case, k)
            assert win.n_files == 0  # the sharded copy job yields no paths
        win.drain()
        assert len(win) == 0
        assert [t for t in log_w if t[0] == 'j'] == [
            ('j', i) for i in range(k + 1)]  # every copy job waited for once, in batch order


def test_window_newest_entry_always_proceeds():
    log = []
    win = InflightWindow(2, 10)
    win.push(Fut(log, 'big', ['a'], 1000), [], 1000)
    win.trim()
    assert log == [] and len(win) == 1  # alone above max_bytes: kept
    win.trim(incoming=1000)
    assert log == ['big'] and len(win) == 0 and win.n_files == 1
    win.push(None, [Fut(log, 'w')], 0)  # no copy job: only the writes are waited for
    win.drain()
    assert log == ['big', 'w'] and win.n_files == 1


def test_window_with_lock_retires_every_entry_once():
    log, lock = [], threading.Lock()
    win = InflightWindow(5, 50, lock)
    n_threads, per_thread = 4, 200

    def pusher(t):
        rng = random.Random(t)
        for i in range(per_thread):
            nb = rng.choice([0, 1, 20, 60])
            tag = (t, i)
            job = [str(tag)] if nb == 0 else Fut(log, ('j',) + tag, [str(tag)], nb)
            win.push(job, [Fut(log, ('w',) + tag)], nb)
            win.trim()
    threads = [threading.Thread(target=pusher, args=(t,)) for t in range(n_threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    win.drain()
    assert len(win) == 0 and win.n_files == n_threads * per_thread
    writes = [x for x in log if x[0] == 'w']
    assert sorted(writes) == sorted(('w', t, i) for t in range(n_threads)
                                    for i in range(per_thread))
    jobs = [x for x in log if x[0] == 'j']
    assert len(jobs) == len(set(jobs))
