"""tools/kernel_coverage.py on the in-tree library (host only: it reads symbol names)."""
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
TOOL = REPO / 'tools' / 'kernel_coverage.py'

KNOWN = ['em_estep_reg_kernel<6, 20, 2>', 'wcov_kernel<2, false, false, false, 1, false>',
         'em_estep_kernel<19, 0>', 'em_onchip4_kernel<2>', 'wpe_corr_persist_kernel<4, false>',
         'wpe_apply_packed_kernel<4, 3, true, 4, 1>', 'mvdr_solve_kernel', 'tri_table_kernel']


@pytest.fixture(scope='module')
def lib():
    from pb_chime5_amd import build
    return build.build(verbose=False)


def _run(*args):
    res = subprocess.run([sys.executable, str(TOOL), *map(str, args)], capture_output=True,
                         text=True)
    assert res.returncode == 0, res.stderr
    return res.stdout


def test_list_names_every_instantiation_once(lib):
    names = _run('list', '--lib', lib).splitlines()
    assert len(names) == len(set(names))            # .symtab and .dynsym list each: one line
    for name in KNOWN:
        assert name in names, name
    # templates come with all their instantiations (at least the ones of today: 5 channel
    # counts x 5 class counts x 2 modes, 19 class counts x 3 modes)
    count = lambda t: sum(n.split('<')[0] == t for n in names)      # noqa: E731
    assert count('em_estep_reg_kernel') >= 50
    assert count('em_estep_kernel') >= 57
    # demangled: no mangled name, no parameter list, no namespace, no descriptor suffix
    assert not [n for n in names if n.startswith('_Z') or '(' in n or n.endswith('.kd')]


def test_diff_names_what_a_trace_never_launched(lib, tmp_path):
    trace = tmp_path / 'run_kernel_trace.csv'
    trace.write_text(
        '"Kind","Agent_Id","Kernel_Name","Start_Timestamp","End_Timestamp"\n'
        '"KERNEL_DISPATCH",1,"void (anonymous namespace)::em_onchip4_kernel<2>((anonymous '
        'namespace)::OnchipArgs)",1,2\n'
        '"KERNEL_DISPATCH",1,"(anonymous namespace)::em_onchip4_kernel<3>((anonymous namespace)'
        '::OnchipArgs) [clone .kd]",3,4\n'
        '"KERNEL_DISPATCH",1,"tri_table_kernel(int, int*)",5,6\n')
    out = _run('diff', trace, '--lib', lib)
    head = out.splitlines()[0]
    assert ' 3 launched' in head, head
    assert 'em_onchip4_kernel: 3 of 5 never launched' in out
    lines = [line.strip() for line in out.splitlines()]
    assert 'em_onchip4_kernel<4>' in lines and 'em_onchip4_kernel<6>' in lines
    assert 'em_onchip4_kernel<2>' not in lines and 'em_onchip4_kernel<3>' not in lines
    assert 'tri_table_kernel' not in lines
    assert 'em_eigh_kernel: 1 of 1 never launched' in out
    # a directory of traces is searched; two traces add up
    more = tmp_path / 'more'
    more.mkdir()
    (more / '7_kernel_trace.csv').write_text(
        '"Kernel_Name"\n"void (anonymous namespace)::em_onchip4_kernel<4>(OnchipArgs)"\n')
    both = _run('diff', trace, more, '--lib', lib)
    assert 'em_onchip4_kernel: 2 of 5 never launched' in both
    # --write-launched: the sorted names of the library's launched instantiations, nothing else
    # (the copy of the kernel from another library that the trace may hold is left out)
    (more / '8_kernel_trace.csv').write_text(
        '"Kernel_Name"\n"void at::native::vectorized_elementwise_kernel<4>(int)"\n')
    out_file = tmp_path / 'launched.txt'
    again = _run('diff', trace, more, '--lib', lib, '--write-launched', out_file)
    assert again.splitlines()[1:3] == both.splitlines()[1:3]
    assert out_file.read_text() == ('em_onchip4_kernel<2>\nem_onchip4_kernel<3>\n'
                                    'em_onchip4_kernel<4>\ntri_table_kernel\n')


# ------------------------------------------------------------------ the record of the suite
LAUNCHED = REPO / 'tests' / 'golden' / 'kernels_launched.txt'
UNREACHABLE = REPO / 'tests' / 'golden' / 'kernels_unreachable.txt'
# entries of kernels_unreachable.txt when the list was written (tests/KERNEL_COVERAGE.md names the
# reason of each): the list may shrink, it must not grow
MAX_UNREACHABLE = 14


def _names(path):
    lines = path.read_text().splitlines()
    assert lines == sorted(set(lines)) and all(line == line.strip() != '' for line in lines), path
    return set(lines)


def test_every_instantiation_is_launched_by_the_gpu_suite_or_listed_as_unreachable(lib):
    """tests/golden/kernels_launched.txt is what a kernel trace of the whole GPU suite launched
    (`diff --write-launched`, tests/KERNEL_COVERAGE.md), kernels_unreachable.txt what no entry
    point can reach.  Together they are the library: a change that adds an instantiation fails
    here until a GPU test launches it and the suite is traced again."""
    names = set(_run('list', '--lib', lib).splitlines())
    launched, unreachable = _names(LAUNCHED), _names(UNREACHABLE)
    assert not launched & unreachable, sorted(launched & unreachable)
    assert len(unreachable) <= MAX_UNREACHABLE
    missing = sorted(names - launched - unreachable)
    assert not missing, f'{len(missing)} instantiations no GPU test is known to launch: {missing}'
    gone = sorted((launched | unreachable) - names)
    assert not gone, f'{len(gone)} recorded names are no longer in the library: {gone}'
