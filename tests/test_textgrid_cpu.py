"""dissc_amd.textgrid on hand-written Praat TextGrid files (tests/golden/textgrid): the long form MFA writes, the short
form of the same grid, and a file with the awkward marks (doubled quotes, brackets, '=', a line break, digits)."""
import os

import pytest

from dissc_amd.textgrid import Interval, TextGrid


def grid(golden_dir, name):
    return TextGrid.fromFile(os.path.join(golden_dir, "textgrid", name))


@pytest.mark.parametrize("name", ["long.TextGrid", "short.TextGrid"])
def test_reads_both_forms_of_the_same_grid(golden_dir, name):
    g = grid(golden_dir, name)
    assert (g.minTime, g.maxTime, len(g)) == (0.0, 1.52, 2)
    words, phones = g[0], g[1]
    assert (words.name, phones.name) == ("words", "phones") and (len(words), len(phones)) == (4, 8)
    assert [(i.minTime, i.maxTime, i.mark) for i in words] == [(0.0, 0.21, ""), (0.21, 0.68, "please"),
                                                              (0.68, 1.3, "call"), (1.3, 1.52, "")]
    assert [i.mark for i in phones if i.mark] == ["P", "L", "IY1", "Z", "K", "AO1 L"]
    assert phones[3].duration() == 0.55 - 0.37 and words.maxTime == 1.52


def test_marks_with_quotes_brackets_and_numbers(golden_dir):
    g = grid(golden_dir, "marks.TextGrid")
    assert g.maxTime == 2.5 and g[0].name == "words 2"
    assert [i.mark for i in g[0]] == ["[laughter] 42", 'she said "hi" = 3\ntwice', "<unk>"]
    assert g[0][0].maxTime == round(0.123456789012345678, 15) == g[0][1].minTime
    assert g[1].is_point and [(p.time, p.mark) for p in g[1]] == [(0.5, "click"), (1.75, "")]


def test_utf16_and_errors(tmp_path, golden_dir):
    text = open(os.path.join(golden_dir, "textgrid", "long.TextGrid"), encoding="utf-8").read()
    p = tmp_path / "u16.TextGrid"
    p.write_bytes(text.replace("please", "s’il").encode("utf-16"))
    assert TextGrid.fromFile(p)[0][1].mark == "s’il"
    with pytest.raises(ValueError):
        TextGrid.fromString("not a grid")
    with pytest.raises(ValueError):
        TextGrid.fromString(text[:text.index("intervals [3]")])
    assert Interval(0.25, 1.0, "a").duration() == 0.75
