"""Vanity addresses: a private key whose base58 address starts with a chosen prefix.

A compressed address is ``b58encode(bytes([42 + parity of y]) + x little-endian)``. Read as a 33-byte big-endian
integer N it lies in [42 * 2**256, 44 * 2**256) and always encodes to 45 characters, so "the address starts with
P" is exactly ``v(P) * 58**(45 - len(P)) <= N < (v(P) + 1) * 58**(45 - len(P))`` with v(P) the base58 value of
P. :func:`prefix_ranges` does that arithmetic; the search (``ops.p256.vanity_search``: K16, csrc/p256_vanity.h)
walks consecutive private keys and compares integers, it never encodes base58.

The walk is not constant-time and its base scalar is a secret: run it on a machine you trust. Whatever it
reports, :func:`find` derives the address again from the private key with the single-key path before it
returns it.
"""
from __future__ import annotations

import secrets
from fractions import Fraction
from typing import Callable, List, Optional, Tuple

from ..ops import p256 as op
from ..ops.native import lib
from ..utils.codec import _B58, _B58_INDEX, point_to_string

ADDRESS_CHARS = 45
SPACE_LO, SPACE_HI = 42 << 256, 44 << 256
Range = Tuple[int, int]


def _variants(c: str, ignore_case: bool) -> List[str]:
    cand = sorted({c.lower(), c.upper()}) if ignore_case else [c]
    ok = [v for v in cand if v in _B58_INDEX]
    if not ok:
        raise ValueError(f'{c!r} is not a base58 character: the alphabet is the digits and letters without '
                         f'0, O, I and l')
    return ok


def _clip(v: int, length: int) -> Optional[Range]:
    """The addresses whose first ``length`` characters have the base58 value v, or None when there are none."""
    unit = 58 ** (ADDRESS_CHARS - length)
    lo, hi = max(v * unit, SPACE_LO), min((v + 1) * unit, SPACE_HI)
    return (lo, hi) if lo < hi else None


def _feasible_starts() -> str:
    parts = []
    for first in _B58:
        if _clip(_B58_INDEX[first], 1):
            second = [c for c in _B58 if _clip(_B58_INDEX[first] * 58 + _B58_INDEX[c], 2)]
            parts.append(f'{first!r} followed by one of {second[0]!r}..{second[-1]!r}')
    return ', or '.join(parts)


def max_ranges() -> int:
    return int(lib().p256_vanity_info()['max_ranges'])


def prefix_ranges(prefix: str, ignore_case: bool = False) -> List[Range]:
    """The sorted, disjoint half-open ranges of the address integer N whose addresses start with ``prefix``
    (in any mix of cases with ``ignore_case``), clipped to the address space, adjacent ranges merged.
    ``ValueError`` for a character outside the alphabet, more than 45 characters, a prefix that no address
    has, or more ranges than one search takes."""
    if not prefix:
        return [(SPACE_LO, SPACE_HI)]
    if len(prefix) > ADDRESS_CHARS:
        raise ValueError(f'an address has {ADDRESS_CHARS} characters, the prefix has {len(prefix)}')
    limit = max_ranges()
    live = [0]  # base58 values of the spellings so far that some address starts with
    for k, c in enumerate(prefix, 1):
        digits = [_B58_INDEX[v] for v in _variants(c, ignore_case)]
        live = [v * 58 + d for v in live for d in digits if _clip(v * 58 + d, k)]
        if not live:
            raise ValueError(f'no address starts with {prefix[:k]!r}: addresses start with {_feasible_starts()}')
        # only the two spellings that straddle an end of the address space can still drop out
        if len(live) - 2 > limit:
            raise ValueError(f'{prefix!r} without case has more than {limit} spellings; use a shorter or an exact prefix')
    merged: List[Range] = []
    for lo, hi in sorted(_clip(v, len(prefix)) for v in live):
        if merged and merged[-1][1] == lo:
            merged[-1] = (merged[-1][0], hi)
        else:
            merged.append((lo, hi))
    if len(merged) > limit:
        raise ValueError(f'{prefix!r} without case needs {len(merged)} ranges, a search takes {limit}')
    return merged


def expected_keys(ranges: List[Range]) -> float:
    """Keys to try on average before one matches: the address space over the ranges' total width."""
    return float(Fraction(SPACE_HI - SPACE_LO, sum(hi - lo for lo, hi in ranges)))


def matches(address: str, prefix: str, ignore_case: bool = False) -> bool:
    return address.lower().startswith(prefix.lower()) if ignore_case else address.startswith(prefix)


def _first_hit(base: int, count: int, ranges: List[Range], device: Optional[str]) -> Optional[int]:
    """The smallest index in [0, count) whose key matches, or None."""
    while True:
        total, idx = op.vanity_search(base, count, ranges, device=device)
        if total == 0:
            return None
        first = int(idx[0])
        if total <= len(idx):
            return first
        count = first + 1  # more hits than were returned: any earlier one lies below the smallest returned


def find(prefix: str, ignore_case: bool = False, device: Optional[str] = None, max_keys: Optional[int] = None,
         base: Optional[int] = None, progress: Optional[Callable[[int, float], None]] = None,
         chunk: Optional[int] = None) -> Optional[Tuple[int, str]]:
    """Walk private keys ``base, base + 1, ...`` (``base`` drawn from ``secrets`` unless given) until one's
    address starts with ``prefix`` -> ``(private key, address)``; None after ``max_keys`` keys. The walk goes
    launch by launch (``chunk`` keys per call, by default one GPU launch or 2**18 keys on the host), calling
    ``progress(keys done, expected keys)`` between them. The address is derived again from the private key
    with ``ops.p256.public_key``; ``RuntimeError`` if that disagrees with the walk."""
    ranges = prefix_ranges(prefix, ignore_case)
    expect = expected_keys(ranges)
    if max_keys is not None and max_keys < 0:
        raise ValueError('max_keys must not be negative')
    if base is None:  # leave room for the walk below n
        base = 1 + secrets.randbelow(op.oracle.N - 1 - (max_keys if max_keys is not None else 1 << 80))
    if not 1 <= base < op.oracle.N:
        raise ValueError('base out of range')
    if chunk is None:
        chunk = int(lib().p256_vanity_info()['keys_per_launch']) if op.vanity_on_gpu(device) else 1 << 18
    done = 0
    while True:
        count = min(chunk, op.oracle.N - base - done)
        if max_keys is not None:
            count = min(count, max_keys - done)
        if count <= 0:
            return None
        i = _first_hit(base + done, count, ranges, device)
        if i is not None:
            d = base + done + i
            address = point_to_string(op.public_key(d))
            if not matches(address, prefix, ignore_case):
                raise RuntimeError(f'the walk reported index {done + i}, whose address {address} does not start '
                                   f'with {prefix!r}')
            return d, address
        done += count
        if progress is not None:
            progress(done, expect)


def progress_line(prefix: str, ignore_case: bool = False) -> str:
    return f'expected keys to try for {prefix!r}: {expected_keys(prefix_ranges(prefix, ignore_case)):.3g}'


def progress_printer(every_s: float = 5.0, file=None) -> Callable[[int, float], None]:
    """A ``progress`` callback for :func:`find` that prints a line at most every ``every_s`` seconds."""
    import sys
    import time
    start = last = time.monotonic()

    def report(done: int, expect: float) -> None:
        nonlocal last
        now = time.monotonic()
        if now - last >= every_s:
            last = now
            print(f'{done:.3g} keys tried ({done / expect:.2f} of the expected number), '
                  f'{done / max(now - start, 1e-9):.3g} keys/s', file=file or sys.stderr, flush=True)
    return report


__all__ = ['prefix_ranges', 'expected_keys', 'find', 'matches', 'max_ranges', 'progress_line', 'progress_printer',
           'SPACE_LO', 'SPACE_HI']
