"""The staleness lists of zbot_lab_amd/build.py against the sources' own #include lines.

zbot_sim.hip is the root of one translation unit whose text lives in pieces beside it; a piece that
build.sim_deps() misses would leave a stale libzbot.so loaded silently, and a piece that the root does
not reach is dead text. Reads files only: no GPU, no built library, no compiler."""
import os
import re

from zbot_lab_amd import build

CSRC = os.path.dirname(build.SRC)
INCLUDE = os.path.join(build.ROOT, "include")
QUOTED = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def reached(root):
    """Every file the quoted #include lines reach from root (root included), each resolved against
    the including file's folder, then include/."""
    seen, todo = set(), [os.path.abspath(root)]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            names = QUOTED.findall(f.read())
        for name in names:
            found = [p for p in (os.path.join(os.path.dirname(path), name), os.path.join(INCLUDE, name)) if os.path.isfile(p)]
            assert found, f"{path} includes {name}, found neither beside it nor under include/"
            todo.append(os.path.abspath(found[0]))
    return seen


def test_sim_deps_cover_every_included_file():
    got = reached(build.SRC)
    assert os.path.abspath(os.path.join(INCLUDE, "zbot.h")) in got and os.path.abspath(os.path.join(CSRC, "zbot_m_step.inc")) in got
    missing = got - {os.path.abspath(d) for d in build.sim_deps()}
    assert not missing, f"included by zbot_sim.hip but not in build.sim_deps(): {sorted(missing)}"
    assert os.path.abspath(build.__file__) in build.sim_deps()


def test_no_orphaned_simulator_piece():
    got = reached(build.SRC)
    files = {os.path.abspath(os.path.join(d, f)) for d, _, fs in os.walk(CSRC) for f in fs}
    orphans = files - got - {os.path.abspath(build.PPO_SRC)}
    assert not orphans, f"under csrc/ but not reached from zbot_sim.hip: {sorted(orphans)}"


def test_ppo_deps_cover_every_included_file():
    got = reached(build.PPO_SRC)
    assert os.path.abspath(os.path.join(INCLUDE, "zbot_ppo.h")) in got
    missing = got - {os.path.abspath(d) for d in build.ppo_deps()}
    assert not missing, f"included by ppo_mlp.hip but not in build.ppo_deps(): {sorted(missing)}"
    assert os.path.abspath(build.__file__) in build.ppo_deps()
