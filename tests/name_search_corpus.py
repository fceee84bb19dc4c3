"""Patterns and names shared by test_name_search.py (DFA against `re` on the
CPU) and test_gpu_name_search.py (device matcher against the host path)."""
import random

# compile with ascii_only=True (declining one of these is a failure)
MUST_COMPILE_ASCII = [
    "ma", "CoA", r"^mus\d\d\d$", "", "^n1", "7$", r"^n\d+$", "a|b", "(ab)+c", "(?:ab)+?c", "[A-Z][a-z]*", "[^a]b",
    ".", "a.c", "x{2,4}", r"\.", "a?b", r"\w+\s\w+", "^$", r"a\Z", "é",
]
# byte-safe: compile with ascii_only=False too
MUST_COMPILE_ANY = ["ma", "é", "^n1", "[A-Z][a-z]*", r"a\Z"]
# not byte-safe: None with ascii_only=False
DECLINE_NON_ASCII = [".", r"\d", "[^a]b", "7$"]
# None whatever the names are
DECLINE_ALWAYS = [r"(a)\1", "(?i)ma", "a(?=b)", r"\bma\b", "(a|b)*a(a|b){16}"]

# further patterns for the differential checks (each either compiles or declines; both answers must be exact)
EXTRA = [
    "^a", "a$", "^a$", r"\Aa", "b+", "a*", "(a|b)*c", "a{3}", "a{2,}", "[a-c]+0", "[0-9]{2}", r"\D", r"\W", r"\S\s",
    "[^0-9]", r"[\d_]x", "^(a|^b)c", "(^a|b$)", "(a$|b)c?", "^$|^a", "(?:)", "a^b", "a$b", r"\s$", r"[^\n]", "naïve",
    "[é]", "[^é]", "٣", "ab|", "x*^a", r"a\Z$",
]

ALL_PATTERNS = list(dict.fromkeys(MUST_COMPILE_ASCII + MUST_COMPILE_ANY + DECLINE_NON_ASCII + DECLINE_ALWAYS + EXTRA))


def names(n_random=2000, seed=7):
    fixed = ["", "a", "b", "7", " ", "mus123", "mus1234", "xmus123", "a\n", "CoA", "acetyl-CoA", "human", "mammal",
             "animal", "é", "naïve", "٣", "n1", "n17", "n1234567", "ab c", "Ab", "abab" * 75]
    rng = random.Random(seed)
    alphabet = "ab c07mZ_.\tx"
    out = list(fixed)
    for _ in range(n_random):
        out.append("".join(rng.choice(alphabet) for _ in range(rng.randint(0, 8))))
    return out


def is_plain_ascii(name):
    b = name.encode("utf-8")
    return all(c < 0x80 and c != 0x0A for c in b)
