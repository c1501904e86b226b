"""Playing: move selection (select.py), the live game and move policy (game.py), the GTP
front end (gtp.py) and lock-step batched self-play / matches (selfplay.py)."""
