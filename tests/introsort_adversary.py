"""The depth-limit fallback of stage B1's sort replay (`deep` in cc_b1_sort, csrc/k_check.h): a CPU search for key sequences on
which libstdc++'s introsort loop exhausts its depth limit 2 * floor(log2 n) while a segment of more than 16 elements is left.

intro_loop() restates std::__introsort_loop (median of three to the front, unguarded Hoare partition, the right part recursed into,
the left part looped on) on a comparison callback and reports whether some segment met depth 0.  adversary() is McIlroy's ("A killer
adversary for quicksort", 1999): keys are undecided ("gas") until compared, a comparison of two gas keys freezes one -- the one
that was the other operand of the last comparison with a frozen key, i.e. the likely pivot -- at the next small value, so every
pivot is among the smallest keys of its segment and a partition peels off one or two elements.
Budget: every n from 17 to 40 (40 keys are free per check: one tgt point per layer against 10 src points), one adversary run each
(deterministic), then for each n that is reached twelve ways of laying ties over the sequence (ranks divided by 2 and 3, shifted,
and folded), each re-checked with plain comparisons.  usage: python tests/introsort_adversary.py; tests/constell_cases.py builds its `deep` slots from adversary() and TIES"""
import sys


def intro_loop(n, less):
    """-> (deep, perm): whether the depth limit ran out on a segment of more than 16, and the arrangement left behind"""
    a = list(range(n))
    hit = []

    def med3(r, x, y, z):
        if less(a[x], a[y]):
            m = y if less(a[y], a[z]) else (z if less(a[x], a[z]) else x)
        else:
            m = x if less(a[x], a[z]) else (z if less(a[y], a[z]) else y)
        a[r], a[m] = a[m], a[r]

    def part(first, last, piv):
        while True:
            while less(a[first], a[piv]):
                first += 1
            last -= 1
            while less(a[piv], a[last]):
                last -= 1
            if not first < last:
                return first
            a[first], a[last] = a[last], a[first]
            first += 1

    def loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                hit.append((first, last))
                return
            depth -= 1
            med3(first, first + 1, first + (last - first) // 2, last - 1)
            cut = part(first + 1, last, first)
            loop(cut, last, depth)
            last = cut
    loop(0, n, 2 * (n.bit_length() - 1))
    return bool(hit), a


def adversary(n):
    gas = n
    val = [gas] * n
    st = {"solid": 0, "cand": 0}

    def less(x, y):
        if val[x] == gas and val[y] == gas:
            z = x if x == st["cand"] else y
            val[z] = st["solid"]
            st["solid"] += 1
        if val[x] == gas:
            st["cand"] = x
        elif val[y] == gas:
            st["cand"] = y
        return val[x] < val[y]
    intro_loop(n, less)
    for i in range(n):          # keys never frozen were never compared with each other: any distinct large values do
        if val[i] == gas:
            val[i] = st["solid"]
            st["solid"] += 1
    return val


def deep_on(keys):
    return intro_loop(len(keys), lambda x, y: keys[x] < keys[y])[0]


TIES = {"distinct": lambda v, n: v, "pairs": lambda v, n: v // 2, "pairs, shifted": lambda v, n: (v + 1) // 2, "triples": lambda v, n: v // 3,
        "top half equal": lambda v, n: min(v, n // 2), "top quarter equal": lambda v, n: min(v, 3 * n // 4),
        # ties laid over sorted positions 8, 9 | 10: which entries are the ninth and tenth of the constellation decides the shaft
        "ranks 7..12 equal": lambda v, n: 7 if 7 <= v <= 12 else v, "ranks 5..14 equal": lambda v, n: 5 if 5 <= v <= 14 else v,
        "ranks 8..10 equal": lambda v, n: 8 if 8 <= v <= 10 else v, "ranks 9..20 equal": lambda v, n: 9 if 9 <= v <= 20 else v,
        "bottom pairs": lambda v, n: v // 2 if v < n // 2 else v, "top pairs": lambda v, n: v if v < n // 2 else n // 2 + (v - n // 2) // 2}

if __name__ == "__main__":
    found = {}
    for n in range(17, 41):
        v = adversary(n)
        assert sorted(v) == list(range(n))
        if deep_on(v):
            found[n] = v
    print("depth limit exhausted for n =", sorted(found) or "none")
    for n in sorted(found)[-3:]:
        for name, f in TIES.items():
            k = [f(x, n) for x in found[n]]
            print("n = %d, %-18s deep = %d  keys = %s" % (n, name, deep_on(k), k))
    sys.exit(0 if found else 1)
