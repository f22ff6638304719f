"""Print glibc's __exp2f_data table (the 32 words the host expf uses) and say where it comes from.

The constants of cmsis-dsp_amd/csrc/host_expf.hpp come from here.  The table is computed from its definition,
T[i] = bits(2^(i/32) correctly rounded to double) - (i << 47), and then looked for in the installed libm's read-only
data (struct exp2f_data begins with uint64_t tab[32]); the tool says whether the libm holds the very same words and
prints the constants that follow them there.  glibc 2.35 (Ubuntu 2.35-0ubuntu3.x) is the version pinned by this image;
tools/expf_check.cpp then proves the restatement equal to the host expf for every float input."""
import struct
import sys
from decimal import Decimal, getcontext

LIBM = sys.argv[1] if len(sys.argv) > 1 else "/lib/x86_64-linux-gnu/libm.so.6"
getcontext().prec = 80
tab = []
for i in range(32):
    v = float(Decimal(2) ** (Decimal(i) / Decimal(32)))      # decimal -> double rounds to nearest
    tab.append(struct.unpack("<Q", struct.pack("<d", v))[0] - (i << 47))
for k in range(0, 32, 4):
    print(" ".join(f"0x{w:016x}ull," for w in tab[k:k + 4]))
try:
    b = open(LIBM, "rb").read()
except OSError:
    sys.exit(f"{LIBM}: not readable; the table above is from the formula alone")
at = b.find(struct.pack("<32Q", *tab))
if at < 0:
    sys.exit(f"{LIBM}: holds no such table")
rest = struct.unpack("<9d", b[at + 256:at + 256 + 72])
print(f"{LIBM}: the same 32 words at offset {at:#x}")
print("shift_scaled", rest[0].hex(), "poly", [p.hex() for p in rest[1:4]])
print("shift", rest[4].hex(), "invln2_scaled", rest[5].hex(), "poly_scaled", [p.hex() for p in rest[6:9]])
