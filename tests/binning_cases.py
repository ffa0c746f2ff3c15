"""What the binning tests share (test infrastructure, not product): the pre-order numbering of a tree given as {TaxId: parent TaxId}
(0: under the virtual root) — the plan of kmcp_amd/csrc/bin_rule.hpp built independently in Python — and an LCA by ancestor sets."""
import numpy as np


def preorder(parent):
    """(parent[], last[], taxid[], node number by TaxId): children in TaxId order, node 0 the virtual root"""
    kids = {}
    for t, p in parent.items():
        kids.setdefault(p, []).append(t)
    par, tax, num = [0], [0], {0: 0}
    stack = [(0, iter(sorted(kids.get(0, []))))]
    last = {}
    while stack:
        v, it = stack[-1]
        t = next(it, None)
        if t is None:
            last[v] = len(par) - 1
            stack.pop()
            continue
        num[t] = len(par)
        par.append(v)
        tax.append(t)
        stack.append((num[t], iter(sorted(kids.get(t, [])))))
    n = len(par)
    return np.array(par, dtype=np.uint32), np.array([last[v] for v in range(n)], dtype=np.uint32), np.array(tax, dtype=np.uint32), num


def ancestors(t, parent):
    """t, its parent, ... and the virtual root 0"""
    out = [t]
    while t != 0:
        t = parent[t]
        out.append(t)
    return out


def lca_of(ids, parent):
    """the deepest common member of the ancestor sets of the TaxIds `ids` (not empty) in the tree `parent`"""
    sets = [set(ancestors(t, parent)) for t in ids]
    return next(a for a in ancestors(ids[0], parent) if all(a in s for s in sets))
