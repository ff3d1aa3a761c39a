"""The host replay of the quote recorder (csrc/cda_quotes.inc k_quote_record) plus the readers' lazy roll, in plain numpy: per market one meta row
(quotes.new_meta) and the flat list of every record written, in record number order.  It states nothing itself - the episode rule is quotes.roll, a visit is
quotes.record, what a ring still holds is quotes.span - so whoever feeds it a market's clock and its book's top ahead of every step gets, from quotes.py alone,
what quote_series, quote_stats, quote_meta and tape_spreads must answer (tests/test_hip_services_fuzz.py; tests/test_quote_replay_host.py holds it to a
hand-worked sequence)."""
import numpy as np

from gym_continuousdoubleauction_amd import quotes as Q


class QuoteReplay:
    def __init__(self, n_markets, capacity):
        self.n, self.capacity = int(n_markets), int(capacity)
        self.meta = [Q.new_meta() for _ in range(self.n)]
        self.records = [[] for _ in range(self.n)]            # record j of market m: records[m][j] (the ring holds it in slot j % capacity while it holds it)
        self.t_step = [0] * self.n                            # every market's clock as the readers will find it

    def visit(self, m, t_step, row):
        """the recorder's visit of a market whose episode is not over: rolled to t_step, then one record more"""
        self.meta[m] = Q.record(self.meta[m], t_step)
        self.records[m].append(np.asarray(row, np.int32).reshape(Q.QUOTE_WORDS).copy())
        assert len(self.records[m]) == self.meta[m]["n_total"]

    def clock(self, m, t_step):
        """the market's t_step from here on (a step ran, a reset, a restore): what a reader rolls to"""
        self.t_step[m] = int(t_step)

    def rolled(self, m):
        """the meta row a reader sees"""
        return Q.roll(self.meta[m], self.t_step[m])

    def held(self, m, episode="current"):
        """what the ring still holds of an episode: (rows int32 [count, 8] oldest first, count, lost, step0, partial)"""
        sp = Q.span(self.rolled(m), self.capacity, episode)
        rows = np.array(self.records[m][sp["start"]:sp["start"] + sp["count"]], np.int32).reshape(-1, Q.QUOTE_WORDS)
        assert len(rows) == sp["count"]
        return rows, sp["count"], sp["lost"], sp["step0"], sp["partial"]
