#!/bin/bash
# tools/build_variant.sh NAME [hipcc flags...]  ->  build/variants/NAME.so  (A/B builds: WAVEMAMBA_HIP_LIB=build/variants/NAME.so)
# wave_mamba_amd/build.py: build_variant() with the library's own flags + the extra ones; "-slp" as an extra flag drops
# -fno-slp-vectorize (the round-4 code generator, which the ISA lint refuses: that variant is linked without the lint).
set -e
cd "$(dirname "$0")/.."
python -c "
import sys; sys.path.insert(0, '.')
from wave_mamba_amd import build
name, extra = sys.argv[1], sys.argv[2:]
slp = '-slp' in extra
build.build_variant('build/variants/%s.so' % name, extra_flags=[f for f in extra if f != '-slp'],
                    drop_flags=['-fno-slp-vectorize'] if slp else [], id_suffix=name, check=not slp, verbose=True)
print('built build/variants/%s.so (%s)' % (name, ' '.join(extra)))" "$@"
