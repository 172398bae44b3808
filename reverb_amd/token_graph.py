"""Transcripts with alternatives and optional words as left-to-right token graphs (Engine.align_graph / rvb_ctc_align_graph).

A TokenGraph has N token nodes in topological order.  Node j carries a label (a vocab id or ctc_align.WILDCARD), an ordered list of
predecessors (earlier nodes, or -1 for "start") and a final flag: a reading of the transcript is a path from a node with a start
predecessor to a final node.  parse_alternatives builds one from text:

    thanks for {calling|phoning} [um] it is {twenty|two zero} [<star>] goodbye

  {a|b c|}   a choice between word sequences; an empty branch makes the group optional
  [x y]      the same as {x y|}
  nesting is allowed, a backslash escapes { } [ ] | and itself, and the wildcard marker (if one is given) is a word.

Every maximal run of plain text is tokenised on its own, so a group stands between words, never inside one.  Epsilons do not exist
in the graph: build(expression, entry set) returns the exit set, and a node's predecessor list is the entry set it was created with,
nearest node first and -1 last -- the order in which the aligner breaks ties.

The node and arc caps are those of the one-batch calls; long_form=True lifts them (the in-degree cap stays) for the graphs that
Engine.align_graph_long_* / rvb_ctc_align_graph_long_* align inside a moving window.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

from .ctc_align import WILDCARD

MAX_NODES = 8192          # RVB_CTC_GRAPH_MAX_NODES, RVB_CTC_GRAPH_MAX_IN_DEGREE, RVB_CTC_GRAPH_MAX_ARCS of include/rvb.h
MAX_IN_DEGREE = 64
MAX_ARCS = 32768
META = "{}[]|"


class TokenGraph:
    def __init__(self, tokens: Sequence[int], preds: Sequence[Sequence[int]], finals: Sequence[bool],
                 words: Optional[Sequence[str]] = None, long_form: bool = False):
        self.tokens = [int(t) for t in tokens]
        self.preds = [[int(p) for p in ps] for ps in preds]
        self.finals = [bool(f) for f in finals]
        self.words = list(words) if words is not None else [""] * len(self.tokens)
        n = len(self.tokens)
        if n == 0:
            raise ValueError("empty graph: no node")
        if not (len(self.preds) == len(self.finals) == len(self.words) == n):
            raise ValueError("tokens, preds, finals and words must have one entry per node")
        if n > MAX_NODES and not long_form:
            raise ValueError("%d nodes exceed RVB_CTC_GRAPH_MAX_NODES = %d" % (n, MAX_NODES))
        for j, ps in enumerate(self.preds):
            if not ps:
                raise ValueError("node %d: empty predecessor list" % j)
            if len(ps) > MAX_IN_DEGREE:
                raise ValueError("node %d: in-degree %d exceeds RVB_CTC_GRAPH_MAX_IN_DEGREE = %d" % (j, len(ps), MAX_IN_DEGREE))
            if len(set(ps)) != len(ps):
                raise ValueError("node %d: duplicate predecessor" % j)
            if any(p < -1 or p >= j for p in ps):
                raise ValueError("node %d: a predecessor must be -1 (start) or an earlier node" % j)
        if sum(map(len, self.preds)) > MAX_ARCS and not long_form:
            raise ValueError("%d arcs exceed RVB_CTC_GRAPH_MAX_ARCS = %d" % (sum(map(len, self.preds)), MAX_ARCS))
        if not any(self.finals):
            raise ValueError("no final node")
        if not any(-1 in ps for ps in self.preds):
            raise ValueError("no node with a start predecessor")

    def __len__(self) -> int:
        return len(self.tokens)

    @classmethod
    def chain(cls, ids: Sequence[int]) -> "TokenGraph":
        """the graph of a plain transcript: what Engine.align / align_wild align"""
        n = len(ids)
        return cls(ids, [[j - 1] for j in range(n)], [j == n - 1 for j in range(n)])

    def arrays(self):
        """-> (labels int32 [N], pred_off int32 [N + 1], preds int32 [arcs], is_final uint8 [N]) as rvb_ctc_align_graph reads them"""
        off = np.zeros(len(self) + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in self.preds])
        return (np.array(self.tokens, np.int32), off, np.array([p for ps in self.preds for p in ps], np.int32),
                np.array(self.finals, np.uint8))

    def text_of(self, nodes: Sequence[int]) -> str:
        """the reading a path spells: the words of its nodes"""
        return " ".join(self.words[j] for j in nodes if self.words[j])


# ---------------------------------------------------------------- the syntax
def _lex(text: str):
    """-> [(kind, value)]: kind "text" (unescaped plain text) or one of the metacharacters"""
    out, buf, i = [], [], 0
    while i < len(text):
        c = text[i]
        if c == "\\":
            if i + 1 >= len(text) or text[i + 1] not in META + "\\":
                raise ValueError("a backslash escapes one of %s and itself (position %d)" % (" ".join(META), i))
            buf.append(text[i + 1])
            i += 2
            continue
        if c in META:
            if buf:
                out.append(("text", "".join(buf)))
                buf = []
            out.append((c, c))
        else:
            buf.append(c)
        i += 1
    if buf:
        out.append(("text", "".join(buf)))
    return out


def _check_word_boundaries(lexed) -> None:
    for k, (kind, value) in enumerate(lexed):
        if kind != "text":
            continue
        if k + 1 < len(lexed) and lexed[k + 1][0] in "{[" and not value[-1].isspace():
            raise ValueError("a group opens inside the word %r: alternatives stand between words" % value.split()[-1])
        if k > 0 and lexed[k - 1][0] in "}]" and not value[0].isspace():
            raise ValueError("a group closes inside the word %r: alternatives stand between words" % value.split()[0])


def _parse(lexed):
    """-> a sequence: list of ("text", str) and ("choice", [sequence, ...])"""
    pos = 0

    def sequence(closers):
        nonlocal pos
        items = []
        while pos < len(lexed) and lexed[pos][0] not in closers:
            kind, value = lexed[pos]
            if kind == "text":
                items.append(("text", value))
                pos += 1
            elif kind in "{[":
                close = "}" if kind == "{" else "]"
                pos += 1
                branches = [sequence("|" + close)]
                while pos < len(lexed) and lexed[pos][0] == "|":
                    pos += 1
                    branches.append(sequence("|" + close))
                if pos >= len(lexed) or lexed[pos][0] != close:
                    raise ValueError("unbalanced brackets: %r is not closed" % kind)
                pos += 1
                if kind == "[":
                    branches.append([])
                items.append(("choice", branches))
            else:
                raise ValueError("unbalanced brackets: unexpected %r" % kind)
        return items

    seq = sequence("")
    assert pos == len(lexed)
    return seq


def parse_alternatives(text: str, tokenize: Callable[[str], Sequence[int]], wildcard: Optional[str] = None,
                       long_form: bool = False) -> TokenGraph:
    """Text with alternatives -> TokenGraph.  `tokenize` maps a run of plain text to token ids; `wildcard` is the gap marker (a word
    of the text) that becomes a node labelled WILDCARD.  graph.words has one entry per node: the text of the run a node opens (the
    marker for a wildcard), "" for the further tokens of a run.  long_form: no node or arc cap (TokenGraph)."""
    if wildcard is not None and (not wildcard or any(c.isspace() for c in wildcard)):
        raise ValueError("the wildcard marker must be one word")
    lexed = _lex(text)
    _check_word_boundaries(lexed)
    tree = _parse(lexed)
    tokens: List[int] = []
    preds: List[List[int]] = []
    words: List[str] = []

    def add(label: int, entry: List[int], word: str) -> List[int]:
        if len(tokens) >= MAX_NODES and not long_form:
            raise ValueError("more than RVB_CTC_GRAPH_MAX_NODES = %d nodes" % MAX_NODES)
        if len(entry) > MAX_IN_DEGREE:
            raise ValueError("node %d (%r): in-degree %d exceeds RVB_CTC_GRAPH_MAX_IN_DEGREE = %d" % (len(tokens), word, len(entry), MAX_IN_DEGREE))
        tokens.append(int(label))
        preds.append(sorted(entry, reverse=True))          # nearest node first, -1 (start) last
        words.append(word)
        return [len(tokens) - 1]

    def run(piece: str, entry: List[int]) -> List[int]:
        piece = " ".join(piece.split())
        if not piece:
            return entry
        first = True
        for t in tokenize(piece):
            entry = add(t, entry, piece if first else "")
            first = False
        return entry

    def build(seq, entry: List[int]) -> List[int]:
        for kind, value in seq:
            if kind == "text":
                plain: List[str] = []
                for word in value.split():
                    if wildcard is not None and word == wildcard:
                        entry = run(" ".join(plain), entry)
                        plain = []
                        entry = add(WILDCARD, entry, wildcard)
                    else:
                        plain.append(word)
                entry = run(" ".join(plain), entry)
            else:
                exits: List[int] = []
                for branch in value:
                    for x in build(branch, entry):
                        if x not in exits:
                            exits.append(x)
                entry = exits
        return entry

    exits = build(tree, [-1])
    if not tokens or all(x < 0 for x in exits):
        raise ValueError("every path through the text is empty: nothing to align")
    if sum(map(len, preds)) > MAX_ARCS and not long_form:
        raise ValueError("%d arcs exceed RVB_CTC_GRAPH_MAX_ARCS = %d" % (sum(map(len, preds)), MAX_ARCS))
    return TokenGraph(tokens, preds, [j in exits for j in range(len(tokens))], words, long_form)
