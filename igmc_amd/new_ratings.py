"""``--new-ratings FILE``: rating changes applied to the training graph on the device (``engine.Graph.updated``) before
``--recommend`` / ``--rank-eval`` (no reference counterpart: the reference rebuilds its indexers from scratch,
util_functions.py:20-66).  Host-only helpers, pure functions of their arguments.

File format: lines ``user item rating`` separated by whitespace, ``#`` starts a comment, blank lines are skipped.  Ids are in the
dataset's own numbering (the one ``recommendations_*.tsv`` prints); ids beyond the graph create new users / items.  ``rating``
is one of the dataset's ``class_values``, or ``0`` to remove the entry.  Lines are executed in order: the last one of a pair wins."""
import numpy as np


def parse_new_ratings(lines, class_values, name='<new ratings>'):
    """``lines``: an iterable of text lines.  -> ``(users int32, items int32, ratings uint8)`` with ratings as the graph stores
    them (index in ``class_values`` + 1; 0 = remove).  ``ValueError`` names the offending line."""
    values = [float(x) for x in np.asarray(class_values).tolist()]
    users, items, ratings = [], [], []
    for no, line in enumerate(lines, 1):
        text = line.split('#', 1)[0].strip()
        if not text:
            continue
        where = '%s, line %d' % (name, no)
        parts = text.split()
        if len(parts) != 3:
            raise ValueError('%s: expected "user item rating", got %r' % (where, text))
        try:
            u, v = int(parts[0]), int(parts[1])
        except ValueError:
            raise ValueError('%s: user and item are integer ids, got %r %r' % (where, parts[0], parts[1]))
        if not (0 <= u < 2 ** 31 - 1 and 0 <= v < 2 ** 31 - 1):
            raise ValueError('%s: ids must be in [0, 2^31 - 1), got %d %d' % (where, u, v))
        try:
            r = float(parts[2])
        except ValueError:
            raise ValueError('%s: rating %r is not a number' % (where, parts[2]))
        if r == 0:
            code = 0
        elif r in values:
            code = values.index(r) + 1
        else:
            raise ValueError('%s: rating %s is none of the dataset\'s ratings %s (0 removes the entry)' % (
                where, parts[2], ' '.join('%g' % x for x in values)))
        users.append(u)
        items.append(v)
        ratings.append(code)
    return np.asarray(users, np.int32), np.asarray(items, np.int32), np.asarray(ratings, np.uint8)


def read_new_ratings(path, class_values):
    with open(path) as f:
        return parse_new_ratings(f, class_values, name=path)


def grown_sizes(n_users, n_items, users, items):
    """The sizes of the graph after the changes: the present ones, or the greatest id + 1 where that is larger."""
    return (max(int(n_users), int(users.max()) + 1 if len(users) else 0),
            max(int(n_items), int(items.max()) + 1 if len(items) else 0))


def flag_error(new_ratings, recommend, rank_eval, use_features):
    """The argument error of ``--new-ratings`` in this combination of flags, or None."""
    if not new_ratings:
        return None
    if not (recommend and recommend > 0) and not rank_eval:
        return '--new-ratings changes the graph that --recommend / --rank-eval run over: give one of them'
    if use_features:
        return '--new-ratings takes no --use-features: new users and items have no feature rows'
    return None
