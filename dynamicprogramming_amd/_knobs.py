"""
The PI_MI355_* environment knobs the Python package reads: one table, and the only reads of those names from
``os.environ`` in the package (the library's own table: csrc/pi_knobs.cpp; both are listed in INTEGRATION.md,
"Environment knobs").  A knob is read when ``read`` is called, never earlier and never cached.
"""
from __future__ import annotations

import os
import re
from pathlib import Path


def _atoi(value: str) -> int:
    """C's atoi: optional blanks, an optional sign, digits; 0 when there are none."""
    m = re.match(r"\s*([+-]?\d+)", value)
    return int(m.group(1)) if m else 0


# The parse rules; they differ for historical reasons and are kept as they are.
_PARSE = {
    "Text": lambda v: v,                                    # as written
    "Lower": lambda v: v.lower(),                           # case-folded
    "StripLower": lambda v: v.strip().lower(),              # blanks around it dropped, case-folded
    "OffIfString0": lambda v: v != "0",                     # exactly "0": off; any other value or unset: on
    "OffIfZero": lambda v: _atoi(v) != 0,                   # the library's rule of the same name (csrc/pi_knobs.cpp)
}

# name -> (kind, what an unset variable stands for, the line INTEGRATION.md repeats)
KNOBS = {
    "PI_MI355_KERNEL_CACHE": ("Text", str(Path(__file__).resolve().parent / "_kcache"), "directory of the code-object and memory-order caches; default _kcache inside the package; read when the package is imported"),
    "PI_MI355_WHOLE_RUN": ("OffIfString0", "1", "0 = keep the round-by-round loop where a whole run fits one launch; default 1; read at every run"),
    "PI_MI355_ORDER": ("StripLower", "", "memory order of the dimensions: user | auto | a permutation such as 0,2,1,3; default the class's choice; read when a solver is constructed"),
    "PI_MI355_ORDER_CACHE": ("OffIfString0", "1", "0 = measure the memory order of an untuned plugin again instead of using the cached decision; default 1; read when the order is tuned"),
    "PI_MI355_TRANSPORT": ("Lower", "rccl", "transport of a sharded solver that is given none: rccl | p2p, in any case, anything else is a ValueError; default rccl; read when a solver is constructed"),
    "PI_MI355_P2P_FUSED": ("OffIfZero", "1", "0 = the peer-to-peer exchange copies instead of delivering from inside the sweep: off when the value's leading integer is 0 or it has none, on otherwise and when unset; read at plan time"),
    "PI_MI355_EXCHANGE": ("Text", "auto", "exchange of a sharded evaluation: auto | allgather | halo, anything else is a KeyError; default auto; read at plan time"),
    "PI_MI355_OVERLAP": ("OffIfString0", "1", "0 = the halo exchange does not overlap the interior sweep; default 1; read at plan time"),
}


def read(key: str):
    """The knob PI_MI355_<key> as its rule parses it, from the environment as it is now."""
    kind, default, _ = KNOBS["PI_MI355_" + key]
    return _PARSE[kind](os.environ.get("PI_MI355_" + key, default))
