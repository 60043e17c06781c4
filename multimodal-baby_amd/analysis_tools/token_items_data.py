"""``Key``: what the word statistics are grouped by (reference analysis_tools/token_items_data.py).  The reference's table
formatting helpers are not carried over."""
from typing import NamedTuple


class Key(NamedTuple):
    token_id: int
    pos: str
