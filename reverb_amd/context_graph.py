"""Hot-word context biasing lists (the reference's asr/wenet/utils/context_graph.py): `tokenize` and a `ContextGraph` with the
reference's constructor.  Here the object only carries the phrases as token ids and the per-token bonus; the Aho-Corasick automaton
itself is built and walked natively (csrc/search.cpp ContextGraph) once the object is handed to `Engine.set_context_graph`,
`RvbASRModel.decode(context_graph=...)` or `load_model(..., context_path=...)`."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

from .tokenizer import SPACE_MARK, RevBpeTokenizer


def tokenize_lines(lines, symbol_table: Dict[str, int], bpe_model=None) -> List[List[int]]:
    """One phrase per entry of `lines` -> token ids.  Without a BPE model a phrase is cut into characters, a space becoming
    the word-boundary mark; with one, RevBpeTokenizer.text2tokens cuts it (sentencepiece when the model file and the package are
    there, longest match against the unit table otherwise).  A piece the table does not have becomes <unk> if the table has
    that, and is dropped if not; an empty line gives an empty phrase."""
    bpe = RevBpeTokenizer(bpe_model, symbol_table) if bpe_model is not None else None
    phrases = []
    for line in lines:
        line = line.strip()
        if bpe is not None:
            pieces = bpe.text2tokens(line)
        else:
            pieces = [SPACE_MARK if ch == " " else ch for ch in line]
        ids = []
        for p in pieces:
            if p in symbol_table:
                ids.append(symbol_table[p])
            elif "<unk>" in symbol_table:
                ids.append(symbol_table["<unk>"])
        phrases.append(ids)
    return phrases


def tokenize(context_list_path, symbol_table: Dict[str, int], bpe_model=None) -> List[List[int]]:
    """tokenize_lines over the lines of a list file, one phrase per line."""
    with open(context_list_path, "r", encoding="utf8") as fin:
        lines = fin.readlines()
    return tokenize_lines(lines, symbol_table, bpe_model)


class ContextGraph:
    """context_list: the phrases as token-id lists; context_score: the bonus per matched token; num_nodes: trie nodes below the
    root (what the reference counts)."""

    def __init__(self, context_list_path: Optional[str], symbol_table: Optional[Dict[str, int]], bpe_model: str = None,
                 context_score: float = 6.0):
        self.context_score = float(context_score)
        self.context_list = tokenize(context_list_path, symbol_table, bpe_model) if context_list_path is not None else []
        self.num_nodes = self._count_nodes()

    @classmethod
    def from_token_ids(cls, lists: Sequence[Sequence[int]], context_score: float = 6.0) -> "ContextGraph":
        g = cls(None, None, context_score=context_score)
        g.context_list = [[int(t) for t in phrase] for phrase in lists]
        g.num_nodes = g._count_nodes()
        return g

    def _count_nodes(self) -> int:
        return len({tuple(p[:i]) for p in self.context_list for i in range(1, len(p) + 1)})

    def flat(self):
        """(tokens int32 [sum of lengths], lens int32 [phrases]) as rvb_set_context_graph takes them."""
        import numpy as np
        lens = np.array([len(p) for p in self.context_list], np.int32)
        toks = np.array([t for p in self.context_list for t in p], np.int32)
        return toks, lens
