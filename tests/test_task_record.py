"""The task record is laid out once, in include/mocca_model.h (enum MoccaTaskWord); mocca_envs_amd/model.py TASK_RECORD mirrors it."""
import os
import re

from mocca_envs_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_words():
    """(name, first word, words, class) of every enumerator, from the enum and the class / length at the head of its comment."""
    src = open(os.path.join(ROOT, "include", "mocca_model.h")).read()
    body = re.search(r"enum MoccaTaskWord \{(.*?)\};", src, flags=re.S).group(1)
    words = re.findall(r"MOCCA_TW_(\w+)\s*=\s*(\d+),?\s*/\*\s*([fi])\b(?:\s+(\d+)\b)?", body)
    assert len(words) == body.count("MOCCA_TW_"), "an enumerator of MoccaTaskWord has no index or no class in its comment"
    return tuple((name, int(w), int(n or 1), c) for name, w, c, n in words)


def test_header_and_model_agree():
    assert _header_words() == M.TASK_RECORD, "include/mocca_model.h and mocca_envs_amd/model.py lay out the task record differently"


def test_task_words_fit_and_have_one_class():
    cls = {}
    for name, w, n, c in M.TASK_RECORD:
        assert 0 <= w and w + n <= M.TASK_WORDS, name
        for k in range(w, w + n):
            assert cls.setdefault(k, c) == c, f"word {k} is both float and int32"
    assert M.TASK_FLOAT_WORDS == tuple(sorted(k for k, c in cls.items() if c == "f"))
    assert M.TW.EPISODE == 9 and M.TW.APPLIED_GAIN == 21 and M.TW.LAST_ROWS == 23   # set by mocca_create, read by bench.py
