"""The host replay of the depth recorder (csrc/cda_depth.inc k_depth_record) plus the readers' lazy roll, in plain numpy: per market one meta row (the quote
tape's: depth.new_meta) and the flat list of every record written, in record number order.  It states nothing itself - the episode rule is quotes.roll, a visit is
quotes.record, what a ring still holds is quotes.span, all three as depth.py re-exports them - so whoever feeds it a market's clock and its book's ladder ahead of
every step gets, from depth.py alone, what depth_series, depth_meta and the three reductions must answer (tests/test_hip_depth.py; tests/test_depth_host.py
holds it to a hand-worked sequence)."""
import numpy as np

from gym_continuousdoubleauction_amd import depth as D


class DepthReplay:
    def __init__(self, n_markets, capacity, levels):
        self.n, self.capacity, self.levels = int(n_markets), int(capacity), int(levels)
        self.words = D.record_words(levels)
        self.meta = [D.new_meta() for _ in range(self.n)]
        self.records = [[] for _ in range(self.n)]            # record j of market m: records[m][j] (the ring holds it in slot j % capacity while it holds it)
        self.t_step = [0] * self.n                            # every market's clock as the readers will find it

    def visit(self, m, t_step, row):
        """the recorder's visit of a market whose episode is not over: rolled to t_step, then one record more"""
        self.meta[m] = D.record(self.meta[m], t_step)
        self.records[m].append(np.asarray(row, np.int32).reshape(self.words).copy())
        assert len(self.records[m]) == self.meta[m]["n_total"]

    def clock(self, m, t_step):
        """the market's t_step from here on (a step ran, a reset, a restore): what a reader rolls to"""
        self.t_step[m] = int(t_step)

    def rolled(self, m):
        """the meta row a reader sees"""
        return D.roll(self.meta[m], self.t_step[m])

    def held(self, m, episode="current"):
        """what the ring still holds of an episode: (rows int32 [count, words] oldest first, count, lost, step0, partial)"""
        sp = D.span(self.rolled(m), self.capacity, episode)
        rows = np.array(self.records[m][sp["start"]:sp["start"] + sp["count"]], np.int32).reshape(-1, self.words)
        assert len(rows) == sp["count"]
        return rows, sp["count"], sp["lost"], sp["step0"], sp["partial"]

    def reductions(self, m, episode, max_dist, tick, lags, k, half, ofi_lags, bar_steps, depths):
        """the three reductions of what the ring holds of an episode, from the specifications: (profile, imbalance, ofi, info row)"""
        rows, count, lost, step0, partial = self.held(m, episode)
        return (D.profile_from_records(rows, self.levels, max_dist, tick), D.imbalance_from_records(rows, self.levels, lags, k, half),
                D.ofi_from_records(rows, self.levels, ofi_lags, bar_steps, depths, head_lost=bool(lost or partial)), [count, lost, step0, partial])
