"""numpy restatement of the episode monitor (include/trex_monitor.h), written from the header's definition and not from the kernel:
f64 accumulators, the finished envs of a call taken one by one in ascending order, no torch. Monitor(n, window, cols, env_offset) takes apply(reward,
done, reason, cols), reset(mask) and gives state() and summary(). `mistake` plants one of MISTAKES: what
tests/test_monitor_cases_host.py qualifies the cases with."""
import numpy as np

MAXWINDOW, MAXCOLS = 65536, 64
N, RET_MEAN, RET_MIN, RET_MAX, LEN_MEAN, LEN_MIN, LEN_MAX, WIN_REASON, TOTAL, BY_REASON, T, SUMMARY = 0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 16, 17
MISTAKES = ("done_reward_left_out", "length_off_by_one", "ring_by_env_only", "wrap_keeps_first", "mark_counts_as_episode",
            "two_bit_reason_once", "not_zeroed_after_record")


def buckets(reason, once=False):
    """the by_reason buckets a record with this reason counts in"""
    if reason == 0:
        return [0]
    hit = [b for b in (1, 2, 3) if (reason >> (b - 1)) & 1]
    return hit[:1] if once else hit


class Monitor:
    def __init__(self, n, window, cols=0, env_offset=0, mistake=None):
        assert 1 <= window <= MAXWINDOW and 0 <= cols <= MAXCOLS and env_offset + n <= 2 ** 32
        assert mistake is None or mistake in MISTAKES
        self.n, self.W, self.C, self.env_offset, self.mistake = n, window, cols, env_offset, mistake
        self.ret, self.len, self.col = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros((n, cols), np.float64)
        self.episodes = np.zeros(n, np.uint32)
        self.last_return, self.last_length = np.zeros(n, np.float32), np.zeros(n, np.int32)
        self.last_reason, self.last_t = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        self.last_cols = np.zeros((n, cols), np.float32)
        self.t, self.total, self.by_reason = 0, 0, np.zeros(4, np.uint64)
        self.ring_return, self.ring_length = np.zeros(window, np.float32), np.zeros(window, np.int32)
        self.ring_reason, self.ring_env, self.ring_t = np.zeros(window, np.int32), np.zeros(window, np.uint32), np.zeros(window, np.uint32)
        self.ring_cols = np.zeros((window, cols), np.float32)

    def _finish(self, e, reason, records):
        self.last_return[e] = np.float32(self.ret[e])
        self.last_length[e] = self.len[e]
        self.last_reason[e], self.last_t[e] = reason, self.t
        self.last_cols[e] = self.col[e].astype(np.float32)
        self.episodes[e] += 1
        records.append(e)
        if self.mistake != "not_zeroed_after_record":
            self.ret[e], self.len[e] = 0.0, 0
            self.col[e] = 0.0

    def _commit(self, records):
        count = len(records)
        order = records
        if self.mistake == "ring_by_env_only":      # the slot taken from the env's index, not from the running count
            slots = [(self.total + e) % self.W for e in order]
        else:
            slots = [(self.total + j) % self.W for j in range(count)]
        keep = range(count)
        if count > self.W:
            keep = range(self.W) if self.mistake == "wrap_keeps_first" else range(count - self.W, count)
        for j in keep:
            e, s = order[j], slots[j]
            self.ring_return[s], self.ring_length[s], self.ring_reason[s] = self.last_return[e], self.last_length[e], self.last_reason[e]
            self.ring_env[s], self.ring_t[s] = self.env_offset + e, self.last_t[e]
            self.ring_cols[s] = self.last_cols[e]
        for e in order:
            for b in buckets(int(self.last_reason[e]), once=self.mistake == "two_bit_reason_once"):
                self.by_reason[b] += np.uint64(1)
        self.total += count

    def apply(self, reward, done, reason=None, cols=None):
        reward, done = np.asarray(reward, np.float32), np.asarray(done, np.float32)
        reason = np.zeros(self.n, np.int32) if reason is None else np.asarray(reason, np.int32)
        cols = np.zeros((self.n, self.C), np.float32) if cols is None else np.asarray(cols, np.float32).reshape(self.n, self.C)
        records = []
        fin = done != 0
        # (1) for every env; the envs do not depend on one another, so the three sums are taken for all of them at once, each
        # one f64 add of a converted f32 value
        self.ret += np.where(fin & (self.mistake == "done_reward_left_out"), np.float64(0.0), reward.astype(np.float64))
        self.len += 1
        self.col += cols.astype(np.float64)
        for e in np.flatnonzero(fin):            # (2) - (4), in ascending e
            if self.mistake == "length_off_by_one":
                self.len[e] -= 1
            self._finish(e, int(reason[e]), records)
        self._commit(records)
        self.t += 1

    def reset(self, mask=None):
        mask = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        records = []
        for e in np.flatnonzero(mask):
            if self.mistake == "mark_counts_as_episode":
                self._finish(e, 0, records)
            self.ret[e], self.len[e] = 0.0, 0
            self.col[e] = 0.0
        if records:
            self._commit(records)

    def state(self):
        """what trex_batch_monitor_info gives, and the three batch counters"""
        keys = ("ring_return", "ring_length", "ring_reason", "ring_env", "ring_t", "ring_cols", "ret", "len", "episodes", "last_return",
                "last_length", "last_reason", "last_t", "last_cols")
        out = {k: getattr(self, k).copy() for k in keys}
        out.update(total=int(self.total), by_reason=self.by_reason.copy(), t=int(self.t))
        return out

    def summary(self):
        """f64 [SUMMARY + C]; the means are the f64 sums in ring order divided by n"""
        n = min(self.total, self.W)
        out = np.full(SUMMARY + self.C, np.nan, np.float64)
        out[N] = n
        r, l, reason = self.ring_return[:n].astype(np.float64), self.ring_length[:n].astype(np.float64), self.ring_reason[:n]
        if n:
            with np.errstate(invalid="ignore"):
                out[RET_MEAN], out[RET_MIN], out[RET_MAX] = r.sum() / n, r.min(), r.max()
                out[LEN_MEAN], out[LEN_MIN], out[LEN_MAX] = l.sum() / n, l.min(), l.max()
                out[SUMMARY:] = self.ring_cols[:n].astype(np.float64).sum(axis=0) / n
        win = np.zeros(4)
        for x in reason:
            for b in buckets(int(x)):
                win[b] += 1
        out[WIN_REASON:WIN_REASON + 4] = win
        out[TOTAL] = self.total
        out[BY_REASON:BY_REASON + 4] = self.by_reason
        out[T] = self.t
        return out

    def mean_bounds(self):
        """the bound of an n-term f64 sum in any order, per mean: n * 2^-53 * sum|x| / n -> (returns, lengths, columns [C])"""
        n = min(self.total, self.W)
        u = 2.0 ** -53
        r, l = np.abs(self.ring_return[:n].astype(np.float64)), np.abs(self.ring_length[:n].astype(np.float64))
        c = np.abs(self.ring_cols[:n].astype(np.float64))
        return u * r.sum(), u * l.sum(), u * c.sum(axis=0)
