"""Models of the reference's prefix search order, for the ordered select's tests.

Two independent statements of one order:

* ``Trie`` restates the reference's ``src/trie.c``: a node's children are an
  array in creation order (tr_insert appends, src/trie.c:74-95), a child is
  found by a scan of that array (tr_find_next_node, src/trie.c:39-56),
  tr_remove clears ``data`` only (src/trie.c:382-414), and tr_search is a
  pre-order walk from the prefix's node (tr_recurse, src/trie.c:154-176) that
  stops at the limit when the limit is positive (src/trie.c:162).
* ``rule_order`` is the rule the device computes (include/lzf_gpu.h): births
  of key prefixes over all the items, dead ones included, rows of births, and
  the ascending order of the live matches' rows.

``Script`` replays a list of steps -- ``("i", key)``, ``("r", key)``,
``("s", prefix, limit)`` -- on a Trie and, beside it, on a device-store image:
item indices in insert order, an overwrite or a remove killing the key's live
item.  tests/golden/trie_order.json holds such scripts with the search results
recorded from the reference's own trie.c, each result as store indices.

The crafted families are scripts too, so that the fixture, the host twin and
the kernel see the same cases.
"""
import random

import numpy as np

ENC_PLAIN, ENC_NULL = 0x00, 0xFF
PAD = 0xFFFFFFFF


class Trie:
    """src/trie.c: a node is [value, data, children]"""

    def __init__(self):
        self.root = [0, None, []]

    @staticmethod
    def _next(node, value):                                # tr_find_next_node, src/trie.c:39-56
        for child in reversed(node[2]):                    # the scan runs from the youngest: --n >= 0
            if child[0] == value:
                return child
        return None

    def insert(self, key, data):                           # tr_insert, src/trie.c:58-106
        node = self.root
        for v in key:
            child = self._next(node, v)
            if child is None:
                child = [v, None, []]
                node[2].append(child)                      # src/trie.c:83-94: appended, never sorted
            node = child
        old, node[1] = node[1], data
        return old

    def find_node(self, key):                              # tr_find_node, src/trie.c:108-125
        node = self.root
        for v in key:
            node = self._next(node, v)
            if node is None:
                return None
        return node

    def remove(self, key):                                 # tr_remove, src/trie.c:382-414: the node stays
        node = self.find_node(key)
        if node is None or node[1] is None:
            return None
        old, node[1] = node[1], None
        return old

    def search(self, prefix, limit):                       # tr_search, src/trie.c:216-242
        found = []
        start = self.find_node(prefix)
        if start is None:
            return found
        stack = [start]
        while stack:                                       # tr_recurse, src/trie.c:154-176, without the C stack
            node = stack.pop()
            if limit > 0 and len(found) == limit:          # src/trie.c:162
                break
            if node[1] is not None:                        # src/trie.c:188
                found.append(node[1])
            stack.extend(reversed(node[2]))                # src/trie.c:172-175: oldest child first
        return found


def rule_order(keys, live, prefix, limit=-1):
    """The rule of include/lzf_gpu.h over a store image: keys (bytes, in item
    order), live (bools).  Returns (list, live matches, candidates, node words)."""
    plen, birth, cands, words = len(prefix), {}, 0, 0
    for i, k in enumerate(keys):
        if not k.startswith(prefix):
            continue
        cands += 1
        words += len(k) - plen
        for d in range(plen + 1, len(k) + 1):
            birth.setdefault(k[:d], i)
    rows = [(tuple(birth[k[:d]] for d in range(plen + 1, len(k) + 1)), i)
            for i, k in enumerate(keys) if live[i] and k.startswith(prefix)]
    order = [i for _, i in sorted(rows)]                   # a tuple that is a prefix of another sorts first
    return (order[:limit] if limit > 0 else order), len(order), cands, words


class Script:
    """steps replayed on a Trie and on the store image beside it"""

    def __init__(self, steps):
        self.trie, self.keys, self.live, self.at = Trie(), [], [], {}
        self.searches = []                                 # per search step: (store image length, prefix, limit, trie result)
        for st in steps:
            if st[0] == "i":
                key = bytes(st[1])
                i = len(self.keys)
                self.keys.append(key)
                self.live.append(True)
                old = self.trie.insert(key, i)
                if old is not None:
                    self.live[old] = False                 # gbDestroyItem of the overwritten item
                self.at[key] = i
            elif st[0] == "r":
                old = self.trie.remove(bytes(st[1]))
                if old is not None:
                    self.live[old] = False
            else:
                self.searches.append((len(self.keys), list(self.live), bytes(st[1]), int(st[2]),
                                      self.trie.search(bytes(st[1]), int(st[2]))))


def store_arrays(keys, live, shift=0):
    """the device-store arrays of a store image: key bytes packed from `shift`
    on, key_off (u64), key_len (u32), enc (u8)"""
    klen = np.array([len(k) for k in keys], np.uint32)
    koff = (np.concatenate([[0], np.cumsum(klen[:-1], dtype=np.int64)]) + shift).astype(np.uint64)
    blob = np.concatenate([np.zeros(shift, np.uint8), np.frombuffer(b"".join(keys), np.uint8)])
    enc = np.where(np.array(live, bool), ENC_PLAIN, ENC_NULL).astype(np.uint8)
    return blob, koff, klen, enc


# ---- scripts -----------------------------------------------------------------

LIMITS = (-1, 0, 1, 2, 3, 5, 1000)


def random_script(rnd):
    """5-120 steps of inserts, overwrites, removes and searches; keys of 1-6
    bytes over a 3-letter alphabet, prefixes of 1-3 bytes"""
    steps, seen = [], []
    for _ in range(rnd.randint(5, 120)):
        r = rnd.random()
        if r < 0.55 or not seen:
            key = bytes(rnd.choice(b"abc") for _ in range(rnd.randint(1, 6)))
            if seen and rnd.random() < 0.2:
                key = rnd.choice(seen)                     # an overwrite
            seen.append(key)
            steps.append(("i", key))
        elif r < 0.75:
            steps.append(("r", rnd.choice(seen)))
        else:
            prefix = bytes(rnd.choice(b"abc") for _ in range(rnd.randint(1, 3)))
            steps.append(("s", prefix, rnd.choice(LIMITS)))
    return steps


def searches(prefix, matches):
    """the limits the issue names: -1, 0, 1, k, matches and matches + 1"""
    return [("s", prefix, lim) for lim in sorted({-1, 0, 1, max(1, matches // 2), max(1, matches), matches + 1})]


def family(name):
    """a crafted family as (steps without searches, prefix); the order under
    the prefix differs from ascending index in every one that has matches"""
    rnd = random.Random("trie-order " + name)
    if name == "dead-birth-deleted":
        # p:b is older than p:a only through p:bz, deleted since; p:b itself came last
        return [("i", b"p:bz"), ("i", b"p:a"), ("i", b"p:b"), ("r", b"p:bz")], b"p:"
    if name == "dead-birth-overwritten":
        # p:b was overwritten: its first item is dead, its node kept its place before p:a
        return [("i", b"q:x"), ("i", b"p:b"), ("i", b"p:a"), ("i", b"p:b"), ("i", b"p:ab")], b"p:"
    if name == "prefix-key":
        # the key equal to the prefix comes first though inserted last; "p:a" before its extensions
        return [("i", b"p:ab"), ("i", b"p:b"), ("i", b"p:abc"), ("i", b"p:a"), ("i", b"p:")], b"p:"
    if name == "deep-longest-first":
        return [("i", b"k" + b"a" * n) for n in range(64, 0, -1)], b"k"
    if name == "deep-shortest-first":
        # a second chain under an older sibling inserted later, so that index order is not the answer
        return [("i", b"kb")] + [("i", b"k" + b"a" * n) for n in range(1, 65)] + [("i", b"kbb"), ("i", b"kab")], b"k"
    if name == "wide":
        vals = list(range(1, 256))
        rnd.shuffle(vals)
        steps = [("i", b"w" + bytes([v]) + b"zz") for v in vals]
        second = list(vals)
        rnd.shuffle(second)
        return steps + [("i", b"w" + bytes([v])) for v in second], b"w"
    if name == "hot":
        stem = b"h:" + bytes(rnd.choice(b"abcdefgh") for _ in range(28))
        tails = set()
        while len(tails) < 4096:
            tails.add(bytes(rnd.choice(b"0123456789abcdef") for _ in range(rnd.randint(1, 4))))
        tails = sorted(tails)
        rnd.shuffle(tails)
        steps = [("i", stem + t) for t in tails]
        steps += [("r", stem + t) for t in rnd.sample(tails, 300)]
        return steps, stem
    if name == "long":
        stem = bytes(rnd.choice(b"xyz") for _ in range(500))
        return [("i", b"L" + stem + b"bb" + bytes([65 + k]) * 9) for k in (2, 0, 1)] + \
               [("i", b"L" + stem[:300] + b"!" * 211), ("i", b"L" + stem), ("i", b"L" + stem + b"ba")], b"L"
    if name == "none":
        return [("i", b"a1"), ("i", b"b2"), ("i", b"a3")], b"zz"
    if name == "none-live":
        return [("i", b"a1"), ("i", b"b2"), ("i", b"a3"), ("r", b"a1"), ("r", b"a3")], b"a"
    raise KeyError(name)


FAMILIES = ("dead-birth-deleted", "dead-birth-overwritten", "prefix-key", "deep-longest-first", "deep-shortest-first",
            "wide", "hot", "long", "none", "none-live")


def family_script(name):
    steps, prefix = family(name)
    probe = Script(steps + [("s", prefix, -1)])
    return steps + searches(prefix, len(probe.searches[0][4]))
