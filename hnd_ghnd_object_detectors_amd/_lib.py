"""ctypes binding of libhnd_hip.so, derived from its C headers: include/hnd_hip.h, hnd_optim.h (the further optimizer
kinds), hnd_codec.h (the 1 ... 8-bit bottleneck codec) and hnd_qat.h (the fake-quantised bottleneck of the training step),
each with a version of its own, and -- beside those four -- hnd_qrange.h (the fixed quantisation range of the bottleneck)
hnd_entropy.h (the entropy-coded link payload), hnd_qchannel.h (per-channel scales), hnd_qimage.h (per-image scales) and
hnd_istream.h (per-image entropy streams), with versions of their own as well.  parse_header() reads the small grammar those headers use; the struct classes, the enum
dictionaries, the ABI numbers, the symbol tuples and every restype / argtypes below come from what it read, so the headers
are the only place the contract is written down.

The library is the ONLY compute path of this package: if it is missing the import of any
compute module fails loudly (no CPU / eager fallback exists on purpose).
"""
import collections
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HND_LIB_PATH') or os.path.join(_HERE, 'libhnd_hip.so')     # env: kernel experiments
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), 'include')                          # where csrc/Makefile takes them from


class HndLibraryError(RuntimeError):
    pass


# ---- the header reader: comments, `#define NAME <integer>`, `typedef enum`, `typedef struct` and prototypes; anything else
# raises HndLibraryError with the header's name and the line
Header = collections.namedtuple('Header', 'defines enums structs functions')
_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'float': C.c_float,
            'double': C.c_double}
_POINTEES = ('void', 'float', 'double', 'int64_t', 'uint8_t', 'uint16_t', 'unsigned char')      # device buffers: c_void_p
_DIRECTIVE = re.compile(r'#\s*(include\s*<\w+\.h>|ifndef\s+\w+|define\s+\w+)$')                 # read and ignored
_TYPEDEF = re.compile(r'typedef\s+(enum|struct)\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;')
_PROTOTYPE = re.compile(r'([^;{}()]+)\(([^;{}()]*)\)\s*;')
_DECLARATION = re.compile(r'\s*(?:const\s+)?(unsigned\s+char|\w+)(\s*\*+\s*|\s+)(\w+)\s*(\[\d*\])?\s*$')
_ENUMERATOR = re.compile(r'\s*(\w+)\s*=\s*(-?\d+)\s*$')
_SPACE = re.compile(r'\s*')


def parse_header(text, name='<header>'):
    """Header(defines {NAME: int}, enums {tag: {ENUMERATOR: int}}, structs {tag: ctypes.Structure class}, functions
    {name: (restype, [argtypes])}) of one C header"""
    def fail(pos, why):
        raise HndLibraryError('%s:%d: %s' % (name, text.count('\n', 0, pos) + 1, why))

    def blank(m):                                   # keeps every offset, so a position still gives its line
        return re.sub(r'[^\n]', ' ', m.group(0))

    text = re.sub(r'/\*.*?\*/|//[^\n]*', blank, text, flags=re.S)
    if '/*' in text:
        fail(text.index('/*'), 'unterminated comment')
    header = Header({}, {}, {}, {})
    lines, pos, cxx = text.split('\n'), 0, False
    for i, line in enumerate(lines):                # directives, and the extern "C" braces of an #ifdef __cplusplus block
        s = line.strip()
        if s.startswith('#'):
            define = re.match(r'#\s*define\s+(\w+)\s+(-?\d+)$', s)
            if define:
                header.defines[define.group(1)] = int(define.group(2))
            elif s in ('#ifdef __cplusplus', '#endif'):
                cxx = s != '#endif'
            elif not _DIRECTIVE.match(s):
                fail(pos, 'unsupported directive %r' % s)
        if cxx or s.startswith('#'):
            lines[i] = ' ' * len(line)
        pos += len(line) + 1
    text = '\n'.join(lines)

    def declare(decl, pos, kind):
        """(identifier, ctypes type) of a struct 'field', a 'param' or a prototype's name and 'return' type"""
        m = _DECLARATION.match(decl) or fail(pos, 'cannot read the declaration %r' % decl.strip())
        base, stars, ident, array = ' '.join(m.group(1).split()), m.group(2).strip(), m.group(3), m.group(4)
        if array:
            ctype = C.POINTER(C.c_float) if (base, stars, kind) == ('float', '', 'param') else None
        elif not stars:
            ctype = _SCALARS.get(base)
        elif stars == '*' and base in header.structs:
            ctype = C.POINTER(header.structs[base])
        elif stars == '*' and (base in _POINTEES or (base, kind) == ('char', 'return')):
            ctype = C.c_char_p if base == 'char' else C.c_void_p
        else:
            ctype = C.POINTER(C.c_void_p) if (base, stars) == ('void', '**') else None
        return (ident, ctype) if ctype is not None else fail(pos, 'unknown type in %r' % decl.strip())

    pos = _SPACE.match(text).end()
    while pos < len(text):
        m = _TYPEDEF.match(text, pos)
        if m:
            what, tag, body, alias = m.groups()
            if tag != alias or tag in header.enums or tag in header.structs:
                fail(pos, 'typedef %s %s must be declared once, under its own name' % (what, tag))
            if what == 'struct' and body.strip() and not body.rstrip().endswith(';'):
                fail(m.end(3), 'field without a semicolon')
            items = [(i.group(0), m.start(3) + _SPACE.match(body, i.start()).end())            # (text, where it begins)
                     for i in re.finditer(r'[^,]+' if what == 'enum' else r'[^;]+', body) if what == 'enum' or i.group(0).strip()]
            if what == 'enum':
                pairs = [_ENUMERATOR.match(t) or fail(at, 'cannot read the enumerator %r' % t.strip()) for t, at in items]
                header.enums[tag] = {e.group(1): int(e.group(2)) for e in pairs}
            else:
                fields = []
                for stmt, at in items:             # `int32_t n, h, w_;`: plain names after the first declarator
                    first, *rest = stmt.split(',')
                    ident, ctype = declare(first, at, 'field')
                    if rest and ('*' in first or not all(re.match(r'\s*\w+\s*$', r) for r in rest)):
                        fail(at, 'cannot read the declarators %r' % stmt.strip())
                    fields += [(ident, ctype)] + [(r.strip(), ctype) for r in rest]
                header.structs[tag] = type(tag, (C.Structure,), {'_fields_': fields, '__doc__': 'struct ' + tag})
        else:
            m = _PROTOTYPE.match(text, pos) or fail(pos, 'neither a typedef enum / struct nor a prototype')
            fname, restype = declare(m.group(1), pos, 'return')
            if fname in header.functions:
                fail(pos, '%s is declared twice' % fname)
            params = [] if m.group(2).strip() == 'void' else m.group(2).split(',')
            header.functions[fname] = (restype, [declare(p, pos, 'param')[1] for p in params])
        pos = _SPACE.match(text, m.end()).end()
    return header


def _read(fname):
    path = os.path.join(INCLUDE_DIR, fname)
    if not os.path.isfile(path):
        raise HndLibraryError('C header %s not found: the binding of libhnd_hip.so is read from it' % path)
    with open(path) as f:
        return parse_header(f.read(), fname)


def _names(header, tag, prefix):
    """{lower-cased enumerator without its prefix: value} of one enum"""
    if not all(k.startswith(prefix) for k in header.enums[tag]):
        raise HndLibraryError('enum %s: an enumerator without the prefix %s' % (tag, prefix))
    return {k[len(prefix):].lower(): v for k, v in header.enums[tag].items()}


HEADERS = {n: _read(n) for n in ('hnd_hip.h', 'hnd_optim.h', 'hnd_codec.h', 'hnd_qat.h')}
_HIP, _OPTIM, _CODEC, _QAT = HEADERS.values()

ConvDesc, WgradDesc, PackDesc, ImageDesc, BoxesDesc, MsePair, MimicPair = (
    _HIP.structs['hnd_' + n] for n in ('conv_desc', 'wgrad_desc', 'pack_desc', 'image_desc', 'boxes_desc', 'mse_pair', 'mimic_pair'))
OptimDesc = _OPTIM.structs['hnd_optim_desc']
MIMIC_KINDS = _names(_HIP, 'hnd_mimic_kind', 'HND_MIMIC_')
OPTIM_KINDS = _names(_OPTIM, 'hnd_optim_kind', 'HND_OPTIM_')
CONV_TILES = _names(_HIP, 'hnd_conv_tile', 'HND_TILE_')              # what hnd_conv2d_igemm_tile answers
WGRAD_VARIANTS = _names(_HIP, 'hnd_wgrad_variant', 'HND_WGRAD_')     # what hnd_conv2d_wgrad_variant answers
ABI_VERSION, OPTIM_ABI = _HIP.defines['HND_ABI_VERSION'], _OPTIM.defines['HND_OPTIM_ABI']
CODEC_ABI, QAT_ABI = _CODEC.defines['HND_CODEC_ABI'], _QAT.defines['HND_QAT_ABI']
EXPORTED_SYMBOLS, OPTIM_SYMBOLS, CODEC_SYMBOLS, QAT_SYMBOLS = (tuple(sorted(h.functions)) for h in HEADERS.values())
# the fixed quantisation range: a fifth header, kept beside HEADERS (whose four entries and symbol counts are pinned)
QRANGE_HEADER_NAME = 'hnd_qrange.h'
QRANGE_HEADER = _read(QRANGE_HEADER_NAME)
QRANGE_ABI, QRANGE_SYMBOLS = QRANGE_HEADER.defines['HND_QRANGE_ABI'], tuple(sorted(QRANGE_HEADER.functions))
if QRANGE_HEADER.structs or QRANGE_HEADER.enums:
    raise HndLibraryError('%s declares a struct or an enum: it may declare functions only' % QRANGE_HEADER_NAME)

# the entropy-coded link payload: a sixth header, read as hnd_qrange.h is
ENTROPY_HEADER_NAME = 'hnd_entropy.h'
ENTROPY_HEADER = _read(ENTROPY_HEADER_NAME)
ENTROPY_ABI, ENTROPY_SYMBOLS = ENTROPY_HEADER.defines['HND_ENTROPY_ABI'], tuple(sorted(ENTROPY_HEADER.functions))
if ENTROPY_HEADER.structs or ENTROPY_HEADER.enums:
    raise HndLibraryError('%s declares a struct or an enum: it may declare functions only' % ENTROPY_HEADER_NAME)

# per-channel scales for the codec and the fake quantiser: a seventh header, read as hnd_qrange.h is
QCHANNEL_HEADER_NAME = 'hnd_qchannel.h'
QCHANNEL_HEADER = _read(QCHANNEL_HEADER_NAME)
QCHANNEL_ABI, QCHANNEL_SYMBOLS = QCHANNEL_HEADER.defines['HND_QCHANNEL_ABI'], tuple(sorted(QCHANNEL_HEADER.functions))
QCHANNEL_MAX_C = QCHANNEL_HEADER.defines['HND_QCHANNEL_MAX_C']
if QCHANNEL_HEADER.structs or QCHANNEL_HEADER.enums:
    raise HndLibraryError('%s declares a struct or an enum: it may declare functions only' % QCHANNEL_HEADER_NAME)

# per-image scales for the codec and the fake quantiser: an eighth header, read as hnd_qrange.h is
QIMAGE_HEADER_NAME = 'hnd_qimage.h'
QIMAGE_HEADER = _read(QIMAGE_HEADER_NAME)
QIMAGE_ABI, QIMAGE_SYMBOLS = QIMAGE_HEADER.defines['HND_QIMAGE_ABI'], tuple(sorted(QIMAGE_HEADER.functions))
QIMAGE_MAX_N, QIMAGE_PART_BLOCKS = QIMAGE_HEADER.defines['HND_QIMAGE_MAX_N'], QIMAGE_HEADER.defines['HND_QIMAGE_PART_BLOCKS']
if QIMAGE_HEADER.structs or QIMAGE_HEADER.enums:
    raise HndLibraryError('%s declares a struct or an enum: it may declare functions only' % QIMAGE_HEADER_NAME)

# per-image entropy streams with device-built tables: a ninth header, read as hnd_qimage.h is
ISTREAM_HEADER_NAME = 'hnd_istream.h'
ISTREAM_HEADER = _read(ISTREAM_HEADER_NAME)
ISTREAM_ABI, ISTREAM_SYMBOLS = ISTREAM_HEADER.defines['HND_ISTREAM_ABI'], tuple(sorted(ISTREAM_HEADER.functions))
ISTREAM_MAX_N = ISTREAM_HEADER.defines['HND_ISTREAM_MAX_N']
if ISTREAM_HEADER.structs or ISTREAM_HEADER.enums:
    raise HndLibraryError('%s declares a struct or an enum: it may declare functions only' % ISTREAM_HEADER_NAME)

_lib = None


def load():
    """dlopen libhnd_hip.so and declare every entry point; raises if it is missing or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HndLibraryError(
            'libhnd_hip.so not found at %s: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(or make -C hnd_ghnd_object_detectors_amd/csrc). There is no CPU fallback.' % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so) and owns the device tensors this library works
    # on: load it FIRST so libhnd_hip.so binds to that copy.  Loaded the other way round the process holds two HIP
    # runtimes and this library's launches fail with "no ROCm-capable device is detected" (seen when build() and
    # smoke() ran in one process).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for header in list(HEADERS.values()) + [QRANGE_HEADER, ENTROPY_HEADER, QCHANNEL_HEADER, QIMAGE_HEADER,
                                                  ISTREAM_HEADER]:
        for name, (res, args) in header.functions.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise HndLibraryError('libhnd_hip.so does not export %s (stale build?)' % name)
            fn.restype = res
            fn.argtypes = args
    if lib.hnd_abi_version() != ABI_VERSION:
        raise HndLibraryError('libhnd_hip.so ABI %d != expected %d' % (lib.hnd_abi_version(), ABI_VERSION))
    if lib.hnd_optim_abi() != OPTIM_ABI:
        raise HndLibraryError('libhnd_hip.so optimizer ABI %d != expected %d' % (lib.hnd_optim_abi(), OPTIM_ABI))
    if lib.hnd_codec_abi() != CODEC_ABI:
        raise HndLibraryError('libhnd_hip.so codec ABI %d != expected %d' % (lib.hnd_codec_abi(), CODEC_ABI))
    if lib.hnd_qat_abi() != QAT_ABI:
        raise HndLibraryError('libhnd_hip.so fake-quantisation ABI %d != expected %d' % (lib.hnd_qat_abi(), QAT_ABI))
    if lib.hnd_qrange_abi() != QRANGE_ABI:
        raise HndLibraryError('libhnd_hip.so quantisation-range ABI %d != expected %d' % (lib.hnd_qrange_abi(), QRANGE_ABI))
    if lib.hnd_entropy_abi() != ENTROPY_ABI:
        raise HndLibraryError('libhnd_hip.so entropy-coding ABI %d != expected %d' % (lib.hnd_entropy_abi(), ENTROPY_ABI))
    if lib.hnd_qchannel_abi() != QCHANNEL_ABI:
        raise HndLibraryError('libhnd_hip.so per-channel codec ABI %d != expected %d' % (lib.hnd_qchannel_abi(), QCHANNEL_ABI))
    if lib.hnd_qimage_abi() != QIMAGE_ABI:
        raise HndLibraryError('libhnd_hip.so per-image codec ABI %d != expected %d' % (lib.hnd_qimage_abi(), QIMAGE_ABI))
    if lib.hnd_istream_abi() != ISTREAM_ABI:
        raise HndLibraryError('libhnd_hip.so per-image stream ABI %d != expected %d' % (lib.hnd_istream_abi(), ISTREAM_ABI))
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().hnd_last_error_string()
        raise RuntimeError('%s failed (status %d): %s' % (what or 'libhnd_hip call', rc,
                                                          msg.decode() if msg else '?'))
