"""HTTP-only wallet (reference: upow/upow_wallet/nodeless_wallet.py:31-200).

``python -m upow_amd.wallet.nodeless {createwallet,send,balance} [-to R] [-d AMOUNT] [-m MSG]``.
``balance --verify [--peer URL ...]`` does not take the node's word for it: see :func:`verified_balance`.
Keys in ``<data dir>/upow_wallet.json`` ({"private_keys": [...]}). Coin selection follows the reference
(single covering input, else smallest-first up to 255 inputs). Unlike the reference, outputs listed
in ``pending_spent_outputs`` (dicts) are really skipped — the reference compared ``tuple(dict)``
(the key names) and never matched.
"""
from __future__ import annotations

import argparse
import os
import sys
from decimal import Decimal

import httpx

from .. import config
from ..models.transaction import Transaction, TransactionInput, TransactionOutput
from ..ops import p256 as op
from ..utils.codec import point_to_string, sha256, string_to_point
from ..utils.jsonstore import JsonStore
from .builders import string_to_bytes


def node_url() -> str:
    return (os.environ.get('UPOW_WALLET_NODE_URL') or os.environ.get('UPOW_CORE_URL') or 'http://localhost:3006/')\
        .rstrip('/') + '/'


def get_address_info(address: str):
    r = httpx.get(f'{node_url()}get_address_info', params={'address': address, 'transactions_count_limit': 0,
                                                           'show_pending': True}, timeout=10)
    result = r.json()['result']
    pending = {(o['tx_hash'], o['index']) for o in result['pending_spent_outputs'] or []}
    inputs = []
    for o in result['spendable_outputs']:
        if (o['tx_hash'], o['index']) in pending:
            continue
        i = TransactionInput(o['tx_hash'], o['index'])
        i.amount = Decimal(str(o['amount']))
        i.public_key = string_to_point(address)
        inputs.append(i)
    return Decimal(result['balance']), inputs


class VerifyError(Exception):
    """``balance --verify``: the node's answer does not check."""


VERIFY_HELP = ('check every spendable output the node lists against the Merkle root of its UTXO set '
               '(GET /get_utxo_root, POST /get_utxo_proofs), and that root against each --peer: the node can then '
               'neither over-report an amount nor show a spent output as unspent. It can still leave outputs out: '
               'the tree is ordered by outpoint, not by owner, so the proven balance is a lower bound.')


def utxo_commitment(url: str) -> dict:
    """``{root, count, block_hash, height}`` as the node at ``url`` reports it."""
    r = httpx.get(f"{url.rstrip('/')}/get_utxo_root", timeout=10)
    res = r.json()['result']
    return {'root': str(res['root']), 'count': int(res['count']), 'block_hash': res['block_hash'],
            'height': int(res['height'])}


def verified_balance(address: str, peers=()):
    """The balance of ``address`` that the node can PROVE, and the commitment it was proven against.

    The node's root is compared with each peer's: two different answers for the same ``block_hash`` refuse the
    whole run (a peer at another block says nothing and is only counted). Then the node must prove every spendable
    output it listed: present in the tree, in ``unspent_outputs``, not staked, owned by this key, with the amount
    it claimed (ledger/utxo_proof.py, from the entry bytes alone). What this shows: no listed output is spent,
    inflated or somebody else's. What it does not show: that the list is complete. The tree is ordered by
    outpoint, not by owner, so a node can still leave outputs out."""
    from ..constants import SMALLEST
    from ..ledger import utxo_proof
    from ..utils.codec import address_forms
    own = utxo_commitment(node_url())
    agreeing = 0
    for peer in peers:
        theirs = utxo_commitment(peer)
        if theirs['block_hash'] != own['block_hash']:
            continue
        if (theirs['root'], theirs['count']) != (own['root'], own['count']):
            raise VerifyError(f"{peer} reports another UTXO root for block {own['block_hash']}: "
                              f"{theirs['root']} ({theirs['count']}) against {own['root']} ({own['count']})")
        agreeing += 1
    _, inputs = get_address_info(address)
    forms = {str(f) for f in address_forms(address)}
    proven = Decimal(0)
    for at in range(0, len(inputs), 1000):
        chunk = inputs[at:at + 1000]
        r = httpx.post(f'{node_url()}get_utxo_proofs', json={'outpoints': [[i.tx_hash, i.index] for i in chunk]},
                       timeout=30)
        res = r.json()['result']
        if (res['root'], int(res['count']), res['block_hash']) != (own['root'], own['count'], own['block_hash']):
            raise VerifyError('the tip moved between the root and the proofs: run again')
        if len(res['proofs']) != len(chunk):
            raise VerifyError('the node did not answer every outpoint')
        for i, proof in zip(chunk, res['proofs']):
            try:
                entry = utxo_proof.verify_outpoint(bytes.fromhex(own['root']), own['count'], i.tx_hash, i.index, proof)
            except utxo_proof.ProofError as e:
                raise VerifyError(f'{i.tx_hash}:{i.index}: {e}') from None
            if entry is None:
                raise VerifyError(f'{i.tx_hash}:{i.index} is listed as spendable but proven absent')
            if entry['table'] != 'unspent_outputs' or entry['is_stake'] or entry['address'] not in forms or \
                    Decimal(entry['amount']) / SMALLEST != i.amount:
                raise VerifyError(f'{i.tx_hash}:{i.index} is not the output the node listed: {entry}')
            proven += i.amount
    return proven, {**own, 'peers_agreeing': agreeing, 'outputs': len(inputs)}


def create_transaction(private_keys, receiving_address, amount, message: bytes = None, send_back_address=None,
                       push: bool = True) -> Transaction:
    amount = Decimal(amount)
    inputs = []
    for d in private_keys:
        address = point_to_string(op.public_key(d))
        send_back_address = send_back_address or address
        _, addr_inputs = get_address_info(address)
        for i in addr_inputs:
            i.private_key = d
        inputs.extend(addr_inputs)
        if sum(i.amount for i in sorted(inputs, key=lambda x: x.amount)[:255]) >= amount:
            break
    if not inputs:
        raise Exception('No spendable outputs')
    if sum(i.amount for i in inputs) < amount:
        raise Exception("Error: You don't have enough funds")
    chosen = []
    if any(i.amount >= amount for i in inputs):
        for i in sorted(inputs, key=lambda x: x.amount):
            if i.amount >= amount:
                chosen.append(i)
                break
    else:
        for i in sorted(inputs, key=lambda x: x.amount):
            chosen.append(i)
            if sum(x.amount for x in chosen) >= amount:
                break
            if len(chosen) >= 255:
                chosen.pop(0)
    total = sum(i.amount for i in chosen)
    if total < amount:
        raise Exception(f'Consolidate outputs: send {total} upow to yourself')
    tx = Transaction(chosen, [TransactionOutput(receiving_address, amount=amount)], message)
    if total > amount:
        tx.outputs.append(TransactionOutput(send_back_address, total - amount))
    tx.sign(private_keys)
    if push:
        httpx.get(f'{node_url()}push_tx', params={'tx_hex': tx.hex()}, timeout=10)
    return tx


def main(argv=None):
    ap = argparse.ArgumentParser(description='UPOW wallet')
    ap.add_argument('command', choices=['createwallet', 'send', 'balance'])
    ap.add_argument('-to', dest='recipient', required=False)
    ap.add_argument('-d', dest='amount', required=False)
    ap.add_argument('-m', dest='message', required=False)
    ap.add_argument('--verify', action='store_true', help='balance: ' + VERIFY_HELP)
    ap.add_argument('--peer', action='append', default=[], metavar='URL',
                    help='balance --verify: another node whose UTXO root must agree for the same block (repeatable)')
    args = ap.parse_args(argv)
    store = JsonStore(os.environ.get('UPOW_NODELESS_KEY_FILE') or config.data_path('upow_wallet.json'))
    keys = [int(k) for k in store.get('private_keys') or []]
    if args.command == 'createwallet':
        d = op.oracle.gen_private_key()
        store.set('private_keys', keys + [d])
        print(f'Private key: {hex(d)}\nAddress: {point_to_string(op.public_key(d))}')
    elif args.command == 'balance':
        total = 0
        for d in keys:
            address = point_to_string(op.public_key(d))
            if args.verify:
                try:
                    bal, against = verified_balance(address, args.peer)
                except VerifyError as e:
                    print(f'\nAddress: {address}\nREFUSED: {e}')
                    return 1
                print(f'\nAddress: {address}\nProven balance: {bal} ({against["outputs"]} outputs proven against UTXO '
                      f'root {against["root"]}, {against["count"]} entries, block {against["height"]} '
                      f'{against["block_hash"]}; {against["peers_agreeing"]} of {len(args.peer)} peers at that block '
                      f'agree; outputs the node left out cannot show)')
            else:
                bal, _ = get_address_info(address)
                print(f'\nAddress: {address}\nPrivate key: {hex(d)}\nBalance: {bal}')
            total += bal
        print(f'\nTotal {"proven balance" if args.verify else "Balance"}: {total}')
    else:
        if not args.recipient or not args.amount:
            ap.error('send needs -to and -d')
        tx = create_transaction(keys, args.recipient, args.amount, string_to_bytes(args.message))
        print(f'Transaction pushed. Transaction hash: {sha256(tx.hex())}')


if __name__ == '__main__':
    sys.exit(main())
