"""`wenet.utils.context_graph` of the reference -> reverb_amd.context_graph."""
from reverb_amd.context_graph import ContextGraph, tokenize  # noqa: F401
