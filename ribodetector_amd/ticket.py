"""The two types that a chunk carries between Predictor.submit_chunk and collect_chunk (detect.py)."""
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, NamedTuple, Optional

# the order in which collect_chunk runs a ticket's checks, whatever the order the side products were enqueued in: when two faults
# coincide, the run ends with the first one's error
CHECK_ORDER = ("totals", "pairs", "summary", "groups", "regions")
# ... and behind them the checks whose fault is the INPUT's, not a table's: a record that --ubam_output cannot write as a BAM record.
# (A tuple of its own, not one more name in CHECK_ORDER: tests/test_chunk_stage_host.py pins CHECK_ORDER to the five names above.)
LATE_CHECKS = ("ubam",)


@dataclass(slots=True)
class Ticket:
    """One submitted chunk. n: its units (reads or pairs); bounds: the ranks' shard bounds (label gather) or None; labels: the unit
    labels on the device; host: their pinned copy (None under the label gather, whose `finish` returns the gathered labels); done: the
    event behind everything the chunk enqueued; pieces: {key: [detect.Piece]} - key (mate, label): the label pieces of that file (one, or
    one per rank behind the label gather), detect.REPORT / detect.REGIONS: those of the two text files, (mate, detect.SPLIT): the
    grouped pieces of the mate's family files under --split_groups (one per grouped call); chunk: mate 1's chunk. checks: name (one of
    CHECK_ORDER or LATE_CHECKS) -> callable that reads, once `done` has passed, the verdict a side product's kernel wrote into pinned memory, and
    raises on a fault. keep: what is only kept alive until the ticket goes."""
    n: int
    bounds: Optional[list]
    chunk: Any
    labels: Any = None
    host: Any = None
    finish: Optional[Callable] = None
    done: Any = None
    pieces: dict = field(default_factory=dict)
    checks: Dict[str, Callable[[], None]] = field(default_factory=dict)
    keep: tuple = ()

    def run_checks(self):
        for name in CHECK_ORDER + LATE_CHECKS:
            if name in self.checks:
                self.checks[name]()


class RegionRepeat(NamedTuple):
    """--regions: the verdict of a chunk's rd_region_format call (pinned info) and what Predictor._regions_chunk takes to format the
    chunk once more when its lines did not fit"""
    info: Any
    chunks: tuple
    dev_in: list
    plans: list
    lo: int
    hi: int
    pairs: Optional[dict]
