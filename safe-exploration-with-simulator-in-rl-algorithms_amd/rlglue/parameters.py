"""The RL-Glue experiment's settings: the reference's `parameters.txt` (rlglue/parameters.txt), which its agent
(SwimmerAgent.py:243-257), its environment (SwimmerEnvironment.cpp:297-326) and its experiment program
(SwimmerExperiment.cpp:48-60) each read their share of."""
from dataclasses import dataclass, fields
from typing import Tuple

_INT = ("n_seg", "N", "b", "H")


@dataclass
class Parameters:
    """`key value...` lines; the defaults are the file the reference ships."""
    n_seg: int = 3
    direction: Tuple[float, float] = (1.0, 0.0)
    h_global: float = 0.01
    N: int = 1
    b: int = 1
    H: int = 1000
    alpha: float = 0.02
    nu: float = 0.02
    max_u: float = 5.0
    l_i: float = 1.0
    k: float = 10.0
    m_i: float = 1.0

    @classmethod
    def load(cls, path):
        """Read a file in the reference's format: lines in any order, unknown keys and blank lines ignored, a key
        that is missing keeps its default."""
        known = {f.name for f in fields(cls)}
        got = {}
        with open(path, "r") as f:
            for line in f:
                tokens = line.split()
                if not tokens or tokens[0] not in known:
                    continue
                key = tokens[0]
                if key == "direction":
                    got[key] = (float(tokens[1]), float(tokens[2]))
                elif key in _INT:
                    got[key] = int(tokens[1])
                else:
                    got[key] = float(tokens[1])
        return cls(**got)

    def save(self, path):
        """Write the same format (floats as repr, so that load() returns an equal object)."""
        with open(path, "w") as f:
            for fld in fields(self):
                v = getattr(self, fld.name)
                if fld.name == "direction":
                    f.write(f"direction {float(v[0])!r} {float(v[1])!r}\n")
                elif fld.name in _INT:
                    f.write(f"{fld.name} {int(v)}\n")
                else:
                    f.write(f"{fld.name} {float(v)!r}\n")

    def validate(self):
        if not 2 <= self.n_seg <= 8:
            raise ValueError(f"n_seg must be 2..8, not {self.n_seg}")
        if self.N < 1 or self.H < 1 or not 1 <= self.b <= self.N:
            raise ValueError(f"need N >= 1, H >= 1 and 1 <= b <= N, got N={self.N} b={self.b} H={self.H}")
        if not self.max_u >= 0.0:
            raise ValueError(f"max_u must be >= 0 (inf: no clip), not {self.max_u}")
        return self
