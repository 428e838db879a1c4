"""Case builders shared by tests/test_state_digest.py and tests/test_state_digest_gpu.py: the known answers of
the state digest (LtHash16/1024 over key records + payloads, ``upow_amd.ledger.utxo.StateDigest``), seeded
random entries, and a small mined ledger. Not a test file."""
import asyncio
import random
from decimal import Decimal

import numpy as np
import pytest

from upow_amd.ledger.utxo import PAYLOAD_DTYPE

# (txid, index, tag, flags, amount, addr)
A = (bytes(range(32)), 0, 0, 0, 1, bytes([42]) + bytes(range(1, 33)))
B = (bytes(range(32, 64)), 255, 0, 1, 600000000, bytes(range(100, 164)))
C = (b'\xff' * 32, 7, 6, 0, 12345, b'')  # L = 0
C_NOISE = (b'\xff' * 32, 7, 6, 1, 999, b'xyz')  # canonicalised: the digest of C

# set -> (lanes[0:4], lane[1023], short id); computed with hashlib and numpy from the definition
KNOWN = {
    (): ((0, 0, 0, 0), 0, '4577ffd454ce69e51a2270ed607b8d177f6ab4f55a4ab9ee86b35ddf0ec5701e'),
    ('A',): ((26070, 32850, 57441, 7641), 5172, 'c75477d194dae8dfccf51124c0ef15ba6592b7b3e62cd51f80d8549c00a2c72c'),
    ('B',): ((41818, 58637, 24425, 48484), 60684, 'ae5bf37023ce0473a10759302c5d2c7c50c135a99a038404b26068fafc2606f4'),
    ('C',): ((59715, 39545, 44934, 31578), 42120, '171ca47560425b0c0365767be9f81f650a7c04a04f661feb57919f663bb43790'),
    ('A', 'B', 'C'): ((62067, 65496, 61264, 22167), 42440,
                      '6240967130b264ca49cfa3f850b080d1420d54710a2bdf6f430949378e3248a8'),
}
ENTRY = {'A': A, 'B': B, 'C': C}


def arrays(entries):
    """(records n x 40, payloads n) of (txid, index, tag, flags, amount, addr) entries; the payload holds exactly
    what the entry says, canonical or not."""
    n = len(entries)
    recs = np.zeros((n, 40), dtype=np.uint8)
    pay = np.zeros(n, dtype=PAYLOAD_DTYPE)
    for k, (txid, index, tag, flags, amount, addr) in enumerate(entries):
        recs[k, :32] = np.frombuffer(txid, dtype=np.uint8)
        recs[k, 32:36] = np.frombuffer(int(index).to_bytes(4, 'little'), dtype=np.uint8)
        recs[k, 36:40] = np.frombuffer(int(tag).to_bytes(4, 'little'), dtype=np.uint8)
        pay['amount'][k] = amount
        pay['len'][k] = len(addr)
        pay['flags'][k] = flags
        pay['addr'][k, :len(addr)] = np.frombuffer(addr, dtype=np.uint8)
    return recs, pay


def check_known(names, digest):
    """``digest`` is the known answer of the set ``names``: lanes, count and short id as literals."""
    lanes, last, short = KNOWN[tuple(names)]
    assert tuple(int(x) for x in digest.state[:4]) == lanes and int(digest.state[1023]) == last
    assert digest.count == len(names) and digest.hex() == short
    assert len(digest.tobytes()) == 2048 and digest.tobytes()[:2] == lanes[0].to_bytes(2, 'little')


def random_entries(n, seed):
    """n entries with distinct outpoints over all seven tags, both address lengths, payload-less entries
    (about one in eight), the stake flag, and indexes that include 0 and 255."""
    rng = random.Random(seed)
    out, seen = [], set()
    while len(out) < n:
        k = len(out)
        txid = rng.randbytes(32)
        index = (0, 255)[k % 2] if k < 16 else rng.randrange(256)
        if (txid, index) in seen:
            continue
        seen.add((txid, index))
        tag = k % 7 if k < 14 else rng.randrange(7)
        kind = k % 8 if k < 16 else rng.randrange(8)
        if kind == 7:
            out.append((txid, index, tag, 0, 0, b''))
            continue
        addr = bytes([42 + rng.randrange(2)]) + rng.randbytes(32) if kind % 2 else rng.randbytes(64)
        out.append((txid, index, tag, int(tag == 0 and rng.randrange(3) == 0), rng.randrange(1, 1 << 50), addr))
    return out


# ------------------------------------------------------------------------------------------------ ledger
KEY_A = 0x1111111111111111111111111111111111111111111111111111111111111111
KEY_B = 0x2222222222222222222222222222222222222222222222222222222222222222


@pytest.fixture
def chain(monkeypatch):
    """An empty in-memory ledger on the host index at a low start difficulty."""
    from upow_amd.ledger import manager
    from upow_amd.ledger.database import Database
    monkeypatch.setattr(manager, 'START_DIFFICULTY', Decimal('1.5'))
    manager.Manager.difficulty = None
    manager.cache.clear()
    db = asyncio.run(Database.create(utxo_backend='host'))
    yield db
    db.close()


async def small_ledger(chain):
    """A mines four blocks, pays B in the 33-byte form, B stakes, A pays B's 64-byte form with the change sent
    to A's 64-byte form: live entries of both address lengths, with and without the stake flag."""
    from upow_amd import devnet
    from upow_amd.utils.codec import AddressFormat, point_to_string, string_to_point
    from upow_amd.wallet import builders
    a, b = builders.address_of(KEY_A), builders.address_of(KEY_B)
    a_full = point_to_string(string_to_point(a), AddressFormat.FULL_HEX)
    b_full = point_to_string(string_to_point(b), AddressFormat.FULL_HEX)
    base = 1_700_000_000
    for k in range(4):
        await devnet.mine_block(a, ts=base + 1 + k)
    tx = await builders.create_transaction(KEY_A, b, '2.5')
    assert await chain.add_pending_transaction(tx)
    await devnet.mine_block(a, [tx], ts=base + 10)
    stx = await builders.create_stake_transaction(KEY_B, '1')
    assert await chain.add_pending_transaction(stx)
    await devnet.mine_block(a, [stx], ts=base + 11)
    tx2 = await builders.create_transaction(KEY_A, b_full, '1.25', send_back_address=a_full)
    assert await chain.add_pending_transaction(tx2)
    await devnet.mine_block(a, [tx2], ts=base + 12)
