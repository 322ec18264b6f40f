"""The stream classes on the CPU (csrc/mxa_config.h stream_class_of; DESIGN.md §4 "RNG streams"): the
table against the draw sites it is derived from.  The build kernel materialises of an agent's own
stream only what its class can read, so a class moved to head or none, or a new agent_rs() site on a
path such a class can take, would read words that were never made.  This file parses the table and
mxa_kernels.hip and fails until the two agree again:

  * no function that draws from the agent's stream (one that holds an agent_rs() site) is reachable
    from the wakeup or message handler of a type classed head or none, wake_frequency apart;
  * wake_frequency returns before its draw for every none type, and guards the draw of a head type;
  * the builder's draws on agent streams are the listed ones: MOMENTUM (head, one randint through
    the head built before it, with the full stream as the fall-back), MKTMAKER and ZI / HBL (full);
  * an o_observe() outside those handlers (the kernelStopping pass) passes sigma_n = 0.0, which
    returns before the draw.

The call graph is by name over the DEV functions of mxa_kernels.hip: coarser than the compiler's (a
name reaches every overload), so it can only over-report."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-optimal-execution_amd", "csrc")
FULL, HEAD, NONE = "MXA_STREAM_FULL", "MXA_STREAM_HEAD", "MXA_STREAM_NONE"
# sites of agent_rs() that are no draw of a handler: the accessor itself, the look-ahead's twist (a
# head or none stream never asks for it: rs_needs_maint), and the builder (checked on its own below)
NOT_A_DRAW = {"agent_rs", "rng_maint", "build"}
BUILDER_DRAWS = {"first_mom": "AG_MOMENTUM", "first_mk": "AG_MKTMAKER", "first_zi": "AG_ZI"}


def _strip(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def table():
    """{AG_* name: class} of stream_class_of, and the class of its default"""
    src = _strip(open(os.path.join(CSRC, "mxa_config.h")).read())
    body = re.search(r"constexpr int stream_class_of\(int type\)\s*\{\s*switch \(type\) \{(.*?)\n  \}\n", src, re.S).group(1)
    out, pending, default = {}, [], None
    for tok, name, cls in re.findall(r"(case\s+(AG_\w+)\s*:|default\s*:|return\s+(MXA_STREAM_\w+)\s*;)", body):
        if tok.startswith("case"):
            pending.append(name)
        elif tok.startswith("default"):
            pending.append(None)
        else:
            for n in pending:
                if n is None:
                    default = cls
                else:
                    out[n] = cls
            pending = []
    assert not pending and default is not None
    return out, default


def agent_types():
    src = _strip(open(os.path.join(CSRC, "mxa_layout.h")).read())
    body = re.search(r"enum \{ (AG_EXCHANGE = 0.*?)\};", src, re.S).group(1)
    return [n for n, _ in re.findall(r"(AG_\w+)\s*=\s*(\d+)", body)]


def functions():
    """{name: body text} of the DEV functions of mxa_kernels.hip (overloads and template forms of
    one name joined), by brace matching from each definition's opening brace"""
    src = _strip(open(os.path.join(CSRC, "mxa_kernels.hip")).read())
    out = {}
    for m in re.finditer(r"(?m)^[ \t]*(?:template\s*<[^>]*>\s*)?DEV\s+[\w:<>\*&\s,]+?\b(\w+)\s*\(", src):
        i = src.find("{", m.end())
        semi = src.find(";", m.end())
        if i < 0 or (0 <= semi < i):  # a declaration
            continue
        depth, j = 1, i + 1
        while depth:
            c = src[j]
            depth += (c == "{") - (c == "}")
            j += 1
        out[m.group(1)] = out.get(m.group(1), "") + src[i:j]
    return out


def reach(funcs, roots):
    seen, todo = set(), list(roots)
    while todo:
        f = todo.pop()
        if f in seen or f not in funcs:
            continue
        seen.add(f)
        todo += [g for g in set(re.findall(r"\b(\w+)\s*(?:<[^;(){}]*>)?\s*\(", funcs[f])) if g in funcs and g not in seen]
    return seen


def handlers(funcs):
    """{AG_* name: the handlers dispatch() and the event loop call for it}"""
    out = {}
    for t, f in re.findall(r"type == (AG_\w+)\) return (?:\(void\))?(\w+)\(", funcs["dispatch"]):
        out.setdefault(t, set()).add(f)
    for t, f in re.findall(r"rgi\(AF_TYPE\) == (AG_\w+)\) n \+= (\w+)\(", funcs["run"]):  # the in-place cycles
        out.setdefault(t, set()).add(f)
    return out


def test_table_names_every_agent_type_or_defaults_to_full():
    tab, default = table()
    assert default == FULL
    assert set(tab) <= set(agent_types()) and set(tab.values()) == {HEAD, NONE}
    assert {t for t, c in tab.items() if c == HEAD} == {"AG_NOISE", "AG_MOMENTUM"}
    assert {t for t, c in tab.items() if c == NONE} == {"AG_EXCHANGE", "AG_POVMM", "AG_SBMM", "AG_OBI", "AG_DUMMYRL",
                                                        "AG_REPLAY", "AG_TWAP"}


def test_no_draw_site_is_reachable_for_a_head_or_none_type():
    tab, _ = table()
    funcs = functions()
    draws = {f for f, body in funcs.items() if "agent_rs()" in body} - NOT_A_DRAW
    assert {"wake_frequency", "o_observe", "zi_place", "value_wake_head", "mk_place_ladder"} <= draws
    hd = handlers(funcs)
    assert set(hd) >= set(agent_types()) - {"AG_EXCHANGE"} and "ex_receive" in hd["AG_EXCHANGE"]
    for t, cls in tab.items():
        got = reach(funcs, hd[t]) & draws
        assert got <= {"wake_frequency"}, (t, cls, sorted(got))
    # the check sees a draw where there is one: the full classes reach theirs
    assert "value_wake_head" in reach(funcs, hd["AG_VALUE"]) and "zi_place" in reach(funcs, hd["AG_ZI"])
    assert "mk_place_ladder" in reach(funcs, hd["AG_MKTMAKER"]) and "zi_place" in reach(funcs, hd["AG_HBL"])


def test_wake_frequency_returns_early_or_guards():
    tab, _ = table()
    body = functions()["wake_frequency"]
    before, after = body.split("agent_rs()", 1)
    early = set(re.findall(r"type == (AG_\w+)\) return", before))
    falls = set(agent_types()) - early
    funcs = functions()
    hd = handlers(funcs)
    for t, cls in tab.items():
        if cls == NONE:  # a type whose wake_frequency falls through to the draw is at least head
            assert t in early or "wake_frequency" not in reach(funcs, hd[t]), t
    assert "wake_frequency" not in reach(funcs, hd["AG_EXCHANGE"])  # (the one none type without an early return)
    assert {t for t in falls if tab.get(t) == HEAD} == {"AG_NOISE"}
    draw, rest = after.split("agent_rs_put", 1)
    assert re.search(r"rs_randint\(A, 0, 100\);\s*if \(mxa_cfg::stream_class\(CFG, type\) == MXA_STREAM_HEAD\) rs_head_guard\(A\);", draw)


def test_builder_draws_are_the_listed_ones():
    tab, _ = table()
    body = functions()["build"]
    sites = [m.start() for m in re.finditer(r"agent_rs\(\)", body)]
    loops = [(m.start(), m.group(1)) for m in re.finditer(r"for \(int a = P\.(first_\w+);", body)]
    seen = []
    for s in sites:
        first = [name for pos, name in loops if pos < s][-1]
        seen.append(BUILDER_DRAWS[first])
    assert seen == ["AG_MOMENTUM", "AG_MKTMAKER", "AG_ZI"]
    for t in seen:
        assert tab.get(t, FULL) != NONE, t
    # the one head class the builder draws from: its heads first, and the full stream if the draw leaves them
    mom = body[sites[0] - 400:sites[1]]
    assert "heads_range(P.first_mom, P.n_mom)" in mom and "A.p > MXA_MT_N + HW" in mom and "mt_seed(A.key" in mom


def test_observations_outside_the_handlers_draw_nothing():
    funcs = functions()
    hd = handlers(funcs)
    inside = set().union(*[reach(funcs, r) for r in hd.values()])
    for f, body in funcs.items():
        for arg in re.findall(r"\bo_observe(?:<[^>]*>)?\(([^;{]*)\);", body):
            if f not in inside:
                assert arg.rstrip().endswith(", 0.0"), (f, arg)
