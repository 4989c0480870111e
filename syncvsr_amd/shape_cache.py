"""Bookkeeping of engine.TrainStep(native=True, max_shapes > 1): one recorded step list per batch shape, least recently used
first out.  Pure Python (no device work): the engine owns the synchronisation that must precede the release of an evicted list."""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Callable, Hashable, Iterable, Optional


def shape_key(tensors: Iterable[Any]) -> tuple:
    """The key of a batch: per slot (shape, dtype) of a tensor, or the type name of anything else (None, a Python number).
    Two batches with the same key can be replayed from the same recorded list."""
    key = []
    for t in tensors:
        shape, dtype = getattr(t, "shape", None), getattr(t, "dtype", None)
        if shape is not None and dtype is not None:
            key.append((tuple(int(s) for s in shape), str(dtype)))
        else:
            key.append(type(t).__name__)
    return tuple(key)


class ShapeLRU:
    """Entries in least-recently-used order, bounded by a count (`max_entries`) and optionally by a weight (`max_weight`, e.g. the bytes a
    recorded list keeps alive; `weight(value)` reads it).  Nothing is released here: the evicting calls RETURN the (key, value) pairs they
    removed, so that the caller can wait for the device before the last reference goes."""

    def __init__(self, max_entries: int, max_weight: Optional[int] = None, weight: Callable[[Any], int] = lambda v: 0):
        if int(max_entries) < 1:
            raise ValueError("max_entries must be >= 1")
        self.max_entries = int(max_entries)
        self.max_weight = None if max_weight is None else int(max_weight)
        self.weight = weight
        self._d: OrderedDict = OrderedDict()

    def __len__(self) -> int:
        return len(self._d)

    def __contains__(self, key: Hashable) -> bool:
        return key in self._d

    def keys(self) -> list:
        """Least recently used first."""
        return list(self._d.keys())

    def items(self) -> list:
        return list(self._d.items())

    def peek(self, key: Hashable, default=None):
        """The value without touching the order."""
        return self._d.get(key, default)

    def get(self, key: Hashable, default=None):
        """The value, which becomes the most recently used."""
        if key not in self._d:
            return default
        self._d.move_to_end(key)
        return self._d[key]

    def make_room(self) -> list:
        """Evicts least recently used entries until one more fits under `max_entries`."""
        out = []
        while len(self._d) >= self.max_entries:
            out.append(self._d.popitem(last=False))
        return out

    def put(self, key: Hashable, value) -> list:
        """Inserts (or replaces) `key` as the most recently used; -> the entries evicted to respect `max_entries`."""
        out = [] if key in self._d else self.make_room()
        self._d[key] = value
        self._d.move_to_end(key)
        return out

    def total_weight(self) -> int:
        return sum(int(self.weight(v)) for v in self._d.values())

    def shrink(self, keep: Optional[Hashable] = None) -> list:
        """Evicts least recently used entries other than `keep` while the total weight exceeds `max_weight`."""
        if self.max_weight is None:
            return []
        out = []
        total = self.total_weight()
        for k in list(self._d.keys()):
            if total <= self.max_weight:
                break
            if k == keep:
                continue
            v = self._d.pop(k)
            total -= int(self.weight(v))
            out.append((k, v))
        return out

    def pop_all(self) -> list:
        out = list(self._d.items())
        self._d.clear()
        return out
