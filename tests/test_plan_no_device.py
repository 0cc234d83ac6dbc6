"""The answers of all four plan hooks without a device: uaes.plan (ECB, CTR, XTS, GCM in both directions, GCM-SIV, OCB),
uaes.poly1305_plan, uaes.eax_siv_plan and uaes.chain_plan.  With no device to ask, every planner sizes its grids for a
256-CU MI355X (uaesk_cus_or_256, csrc/uaes_launch.hip.h), so a machine without a GPU and an MI355X give the same table.

EXPECTED was recorded from a build of commit 0111e53 ("Plan rows and boundary tests for CBC/CFB/OFB, CMAC, CCM and
batches"), the parent of the change that gave the kernel files one CU count, on a machine without a GPU: the planners
must keep answering what they answered when each file counted the CUs for itself.  None = the hook has no plan for
those arguments (uaes.chain_plan raises ValueError)."""
import pytest

import micro_aes_amd as uaes

MIB, GIB = 1 << 20, 1 << 30
J0 = bytes(range(1, 16)) + b"\x05"          # a GCM J0 / CTR counter block whose low byte is not 0

# sizes 16 B, 4 KiB, 1 MiB, 8 MiB - 16, 8 MiB, 20 MiB, 64 MiB, 1 GiB; batches of 1, 8192, 8193 and 81920 messages of 64 bytes
EXPECTED = [
    ("plan", ("ecb", 16), {}, ("ecb.single", 1, 1, 0)),
    ("plan", ("ecb", 16), {"direction": 1}, ("ecb.single", 1, 1, 0)),
    ("plan", ("ctr", 16), {}, ("ctr.single", 1, 1, 0)),
    ("plan", ("xts", 16, 1), {}, ("xts.small", 1, 1, 0)),
    ("plan", ("gcm", 16), {}, ("gcm.small", 1, 1, 0)),
    ("plan", ("gcm", 16), {"direction": 1}, ("gcm.small", 1, 1, 0)),
    ("plan", ("gcm", 16, 37), {}, ("gcm.small", 1, 1, 0)),
    ("plan", ("gcm", 16), {"counter": J0}, ("gcm.small", 1, 1, 0)),
    ("plan", ("ctr", 16), {"counter": J0}, ("ctr.single", 1, 1, 0)),
    ("plan", ("siv", 16), {}, ("siv.small", 1, 1, 0)),
    ("plan", ("siv", 16), {"direction": 1}, ("siv.small", 1, 1, 0)),
    ("plan", ("ocb", 16), {}, ("ocb.small", 1, 1, 0)),
    ("plan", ("ocb", 16), {"direction": 1}, ("ocb.small", 1, 1, 0)),
    ("poly1305_plan", (16,), {}, ("poly.small", 1, 1, 1)),
    ("eax_siv_plan", (False, 16), {"decrypt": False}, ("eax.small", 1, 1, 16384)),
    ("eax_siv_plan", (False, 16), {"decrypt": True}, ("eax.small", 1, 1, 16384)),
    ("eax_siv_plan", (True, 16), {"decrypt": False}, ("s2v.small", 1, 1, 16384)),
    ("eax_siv_plan", (True, 16), {"decrypt": True}, ("s2v.small", 1, 1, 16384)),
    ("chain_plan", ("cbc", 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", 16), {"decrypt": True}, ("fbdec.single", 1, 1, 1024)),
    ("chain_plan", ("cfb", 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", 16), {"decrypt": True}, ("fbdec.single", 1, 1, 1024)),
    ("chain_plan", ("ofb", 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", 16), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 16), {"decrypt": True}, None),
    ("chain_plan", ("ccm", 16), {"decrypt": False}, ("ccm.fused", 1, 1, 64)),
    ("chain_plan", ("ccm", 16), {"decrypt": True}, ("ccm.fused", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", 16), {"decrypt": True}, ("fbdec.single", 1, 1, 1024)),
    ("plan", ("ecb", 4096), {}, ("ecb.single", 1, 1, 0)),
    ("plan", ("ecb", 4096), {"direction": 1}, ("ecb.single", 1, 1, 0)),
    ("plan", ("ctr", 4096), {}, ("ctr.single", 1, 1, 0)),
    ("plan", ("xts", 4096, 1), {}, ("xts.small", 1, 1, 0)),
    ("plan", ("gcm", 4096), {}, ("gcm.small", 1, 1, 0)),
    ("plan", ("gcm", 4096), {"direction": 1}, ("gcm.small", 1, 1, 0)),
    ("plan", ("gcm", 4096, 37), {}, ("gcm.small", 1, 1, 0)),
    ("plan", ("gcm", 4096), {"counter": J0}, ("gcm.small", 1, 1, 0)),
    ("plan", ("ctr", 4096), {"counter": J0}, ("ctr.single", 1, 1, 0)),
    ("plan", ("siv", 4096), {}, ("siv.small", 1, 1, 0)),
    ("plan", ("siv", 4096), {"direction": 1}, ("siv.small", 1, 1, 0)),
    ("plan", ("ocb", 4096), {}, ("ocb.small", 1, 1, 0)),
    ("plan", ("ocb", 4096), {"direction": 1}, ("ocb.small", 1, 1, 0)),
    ("poly1305_plan", (4096,), {}, ("poly.small", 1, 1, 1)),
    ("plan", ("xts", 4096, 1), {}, ("xts.small", 1, 1, 0)),
    ("plan", ("xts", 512, 8), {}, ("xts.small", 1, 1, 0)),
    ("eax_siv_plan", (False, 4096), {"decrypt": False}, ("eax.small", 1, 1, 16384)),
    ("eax_siv_plan", (False, 4096), {"decrypt": True}, ("eax.small", 1, 1, 16384)),
    ("eax_siv_plan", (True, 4096), {"decrypt": False}, ("s2v.small", 1, 1, 16384)),
    ("eax_siv_plan", (True, 4096), {"decrypt": True}, ("s2v.small", 1, 1, 16384)),
    ("chain_plan", ("cbc", 4096), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", 4096), {"decrypt": True}, ("fbdec.single", 1, 1, 1024)),
    ("chain_plan", ("cfb", 4096), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", 4096), {"decrypt": True}, ("fbdec.single", 1, 1, 1024)),
    ("chain_plan", ("ofb", 4096), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", 4096), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 4096), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 4096), {"decrypt": True}, None),
    ("chain_plan", ("ccm", 4096), {"decrypt": False}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("ccm", 4096), {"decrypt": True}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("cbc_nocts", 4096), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", 4096), {"decrypt": True}, ("fbdec.single", 1, 1, 1024)),
    ("plan", ("ecb", MIB), {}, ("ecb.single", 1, 64, 0)),
    ("plan", ("ecb", MIB), {"direction": 1}, ("ecb.single", 1, 64, 0)),
    ("plan", ("ctr", MIB), {}, ("ctr.single", 1, 64, 0)),
    ("plan", ("xts", MIB, 1), {}, ("xts.small", 1, 64, 0)),
    ("plan", ("gcm", MIB), {}, ("gcm.chunks", 1, 64, 1)),
    ("plan", ("gcm", MIB), {"direction": 1}, ("gcm.chunks", 2, 64, 1)),
    ("plan", ("gcm", MIB, 37), {}, ("gcm.chunks", 1, 65, 1)),
    ("plan", ("gcm", MIB), {"counter": J0}, ("gcm.chunks", 1, 64, 1)),
    ("plan", ("ctr", MIB), {"counter": J0}, ("ctr.single", 1, 64, 0)),
    ("plan", ("siv", MIB), {}, ("siv.chunks", 3, 64, 1)),
    ("plan", ("siv", MIB), {"direction": 1}, ("siv.chunks", 3, 64, 1)),
    ("plan", ("ocb", MIB), {}, ("ocb.runs", 1, 0, 0)),
    ("plan", ("ocb", MIB), {"direction": 1}, ("ocb.runs", 1, 0, 0)),
    ("poly1305_plan", (MIB,), {}, ("poly.chunks", 2, 32, 8)),
    ("plan", ("xts", 4096, 256), {}, ("xts.small", 1, 64, 0)),
    ("plan", ("xts", 512, 2048), {}, ("xts.small", 1, 128, 0)),
    ("eax_siv_plan", (False, MIB), {"decrypt": False}, ("eax.long", 3, 1, 16384)),
    ("eax_siv_plan", (False, MIB), {"decrypt": True}, ("eax.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, MIB), {"decrypt": False}, ("s2v.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, MIB), {"decrypt": True}, ("s2v.long", 2, 1, 16384)),
    ("chain_plan", ("cbc", MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", MIB), {"decrypt": True}, ("fbdec.single", 1, 64, 1024)),
    ("chain_plan", ("cfb", MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", MIB), {"decrypt": True}, ("fbdec.single", 1, 64, 1024)),
    ("chain_plan", ("ofb", MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", MIB), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", MIB), {"decrypt": True}, None),
    ("chain_plan", ("ccm", MIB), {"decrypt": False}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("ccm", MIB), {"decrypt": True}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("cbc_nocts", MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", MIB), {"decrypt": True}, ("fbdec.single", 1, 64, 1024)),
    ("plan", ("ecb", 8 * MIB - 16), {}, ("ecb.single", 1, 256, 0)),
    ("plan", ("ecb", 8 * MIB - 16), {"direction": 1}, ("ecb.single", 1, 256, 0)),
    ("plan", ("ctr", 8 * MIB - 16), {}, ("ctr.single", 1, 256, 0)),
    ("plan", ("xts", 8 * MIB - 16, 1), {}, ("xts.small", 1, 256, 0)),
    ("plan", ("gcm", 8 * MIB - 16), {}, ("gcm.chunks", 1, 256, 2)),
    ("plan", ("gcm", 8 * MIB - 16), {"direction": 1}, ("gcm.chunks", 2, 256, 2)),
    ("plan", ("gcm", 8 * MIB - 16, 37), {}, ("gcm.chunks", 1, 129, 4)),
    ("plan", ("gcm", 8 * MIB - 16), {"counter": J0}, ("gcm.chunks", 1, 256, 2)),
    ("plan", ("ctr", 8 * MIB - 16), {"counter": J0}, ("ctr.single", 1, 256, 0)),
    ("plan", ("siv", 8 * MIB - 16), {}, ("siv.chunks", 3, 256, 2)),
    ("plan", ("siv", 8 * MIB - 16), {"direction": 1}, ("siv.chunks", 3, 256, 2)),
    ("plan", ("ocb", 8 * MIB - 16), {}, ("ocb.runs", 1, 0, 0)),
    ("plan", ("ocb", 8 * MIB - 16), {"direction": 1}, ("ocb.runs", 1, 0, 0)),
    ("poly1305_plan", (8 * MIB - 16,), {}, ("poly.chunks", 2, 256, 8)),
    ("plan", ("xts", 4096, 2047), {}, ("xts.bulk", 2, 0, 0)),
    ("plan", ("xts", 512, 16383), {}, ("xts.packed", 2, 0, 0)),
    ("eax_siv_plan", (False, 8 * MIB - 16), {"decrypt": False}, ("eax.long", 3, 1, 16384)),
    ("eax_siv_plan", (False, 8 * MIB - 16), {"decrypt": True}, ("eax.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 8 * MIB - 16), {"decrypt": False}, ("s2v.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 8 * MIB - 16), {"decrypt": True}, ("s2v.long", 2, 1, 16384)),
    ("chain_plan", ("cbc", 8 * MIB - 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", 8 * MIB - 16), {"decrypt": True}, ("fbdec.single", 1, 256, 1024)),
    ("chain_plan", ("cfb", 8 * MIB - 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", 8 * MIB - 16), {"decrypt": True}, ("fbdec.single", 1, 256, 1024)),
    ("chain_plan", ("ofb", 8 * MIB - 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", 8 * MIB - 16), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 8 * MIB - 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 8 * MIB - 16), {"decrypt": True}, None),
    ("chain_plan", ("ccm", 8 * MIB - 16), {"decrypt": False}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("ccm", 8 * MIB - 16), {"decrypt": True}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("cbc_nocts", 8 * MIB - 16), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", 8 * MIB - 16), {"decrypt": True}, ("fbdec.single", 1, 256, 1024)),
    ("plan", ("ecb", 8 * MIB), {}, ("ecb.single", 1, 256, 0)),
    ("plan", ("ecb", 8 * MIB), {"direction": 1}, ("ecb.single", 1, 256, 0)),
    ("plan", ("ctr", 8 * MIB), {}, ("ctr.single", 1, 256, 0)),
    ("plan", ("xts", 8 * MIB, 1), {}, ("xts.small", 1, 256, 0)),
    ("plan", ("gcm", 8 * MIB), {}, ("gcm.chunks", 1, 256, 2)),
    ("plan", ("gcm", 8 * MIB), {"direction": 1}, ("gcm.chunks", 2, 256, 2)),
    ("plan", ("gcm", 8 * MIB, 37), {}, ("gcm.chunks", 1, 129, 4)),
    ("plan", ("gcm", 8 * MIB), {"counter": J0}, ("gcm.chunks", 1, 256, 2)),
    ("plan", ("ctr", 8 * MIB), {"counter": J0}, ("ctr.single", 1, 256, 0)),
    ("plan", ("siv", 8 * MIB), {}, ("siv.chunks", 3, 256, 2)),
    ("plan", ("siv", 8 * MIB), {"direction": 1}, ("siv.chunks", 3, 256, 2)),
    ("plan", ("ocb", 8 * MIB), {}, ("ocb.runs", 1, 0, 0)),
    ("plan", ("ocb", 8 * MIB), {"direction": 1}, ("ocb.runs", 1, 0, 0)),
    ("poly1305_plan", (8 * MIB,), {}, ("poly.chunks", 2, 256, 8)),
    ("plan", ("xts", 4096, 2048), {}, ("xts.bulk", 2, 0, 0)),
    ("plan", ("xts", 512, 16384), {}, ("xts.packed", 2, 0, 0)),
    ("eax_siv_plan", (False, 8 * MIB), {"decrypt": False}, ("eax.long", 3, 1, 16384)),
    ("eax_siv_plan", (False, 8 * MIB), {"decrypt": True}, ("eax.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 8 * MIB), {"decrypt": False}, ("s2v.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 8 * MIB), {"decrypt": True}, ("s2v.long", 2, 1, 16384)),
    ("chain_plan", ("cbc", 8 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", 8 * MIB), {"decrypt": True}, ("fbdec.single", 1, 256, 1024)),
    ("chain_plan", ("cfb", 8 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", 8 * MIB), {"decrypt": True}, ("fbdec.single", 1, 256, 1024)),
    ("chain_plan", ("ofb", 8 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", 8 * MIB), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 8 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 8 * MIB), {"decrypt": True}, None),
    ("chain_plan", ("ccm", 8 * MIB), {"decrypt": False}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("ccm", 8 * MIB), {"decrypt": True}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("cbc_nocts", 8 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", 8 * MIB), {"decrypt": True}, ("fbdec.single", 1, 256, 1024)),
    ("plan", ("ecb", 20 * MIB), {}, ("ecb.tiled", 1, 256, 0)),
    ("plan", ("ecb", 20 * MIB), {"direction": 1}, ("ecb.tiled", 1, 256, 0)),
    ("plan", ("ctr", 20 * MIB), {}, ("ctr.striped", 1, 256, 0)),
    ("plan", ("xts", 20 * MIB, 1), {}, ("xts.bulk", 3, 0, 0)),
    ("plan", ("gcm", 20 * MIB), {}, ("gcm.twophase", 2, 160, 8)),
    ("plan", ("gcm", 20 * MIB), {"direction": 1}, ("gcm.chunks", 2, 160, 8)),
    ("plan", ("gcm", 20 * MIB, 37), {}, ("gcm.twophase", 2, 161, 8)),
    ("plan", ("gcm", 20 * MIB), {"counter": J0}, ("gcm.twophase", 2, 160, 8)),
    ("plan", ("ctr", 20 * MIB), {"counter": J0}, ("ctr.striped", 1, 256, 0)),
    ("plan", ("siv", 20 * MIB), {}, ("siv.chunks", 3, 160, 8)),
    ("plan", ("siv", 20 * MIB), {"direction": 1}, ("siv.chunks", 3, 160, 8)),
    ("plan", ("ocb", 20 * MIB), {}, ("ocb.runs", 1, 0, 0)),
    ("plan", ("ocb", 20 * MIB), {"direction": 1}, ("ocb.runs", 1, 0, 0)),
    ("poly1305_plan", (20 * MIB,), {}, ("poly.chunks", 2, 640, 8)),
    ("plan", ("xts", 4096, 5120), {}, ("xts.bulk", 2, 0, 0)),
    ("plan", ("xts", 512, 40960), {}, ("xts.packed", 2, 0, 0)),
    ("eax_siv_plan", (False, 20 * MIB), {"decrypt": False}, ("eax.long", 3, 1, 16384)),
    ("eax_siv_plan", (False, 20 * MIB), {"decrypt": True}, ("eax.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 20 * MIB), {"decrypt": False}, ("s2v.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 20 * MIB), {"decrypt": True}, ("s2v.long", 2, 1, 16384)),
    ("chain_plan", ("cbc", 20 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", 20 * MIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("chain_plan", ("cfb", 20 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", 20 * MIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("chain_plan", ("ofb", 20 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", 20 * MIB), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 20 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 20 * MIB), {"decrypt": True}, None),
    ("chain_plan", ("ccm", 20 * MIB), {"decrypt": False}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("ccm", 20 * MIB), {"decrypt": True}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("cbc_nocts", 20 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", 20 * MIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("plan", ("ecb", 64 * MIB), {}, ("ecb.tiled", 1, 256, 0)),
    ("plan", ("ecb", 64 * MIB), {"direction": 1}, ("ecb.tiled", 1, 256, 0)),
    ("plan", ("ctr", 64 * MIB), {}, ("ctr.striped", 1, 256, 0)),
    ("plan", ("xts", 64 * MIB, 1), {}, ("xts.bulk", 3, 0, 0)),
    ("plan", ("gcm", 64 * MIB), {}, ("gcm.twophase", 2, 256, 16)),
    ("plan", ("gcm", 64 * MIB), {"direction": 1}, ("gcm.chunks", 2, 256, 16)),
    ("plan", ("gcm", 64 * MIB, 37), {}, ("gcm.twophase", 2, 129, 32)),
    ("plan", ("gcm", 64 * MIB), {"counter": J0}, ("gcm.twophase", 2, 256, 16)),
    ("plan", ("ctr", 64 * MIB), {"counter": J0}, ("ctr.striped", 1, 256, 0)),
    ("plan", ("siv", 64 * MIB), {}, ("siv.chunks", 3, 256, 16)),
    ("plan", ("siv", 64 * MIB), {"direction": 1}, ("siv.chunks", 3, 256, 16)),
    ("plan", ("ocb", 64 * MIB), {}, ("ocb.runs", 1, 0, 0)),
    ("plan", ("ocb", 64 * MIB), {"direction": 1}, ("ocb.runs", 1, 0, 0)),
    ("poly1305_plan", (64 * MIB,), {}, ("poly.chunks", 2, 2048, 8)),
    ("plan", ("xts", 4096, 16384), {}, ("xts.bulk", 2, 0, 0)),
    ("plan", ("xts", 512, 131072), {}, ("xts.packed", 2, 0, 0)),
    ("eax_siv_plan", (False, 64 * MIB), {"decrypt": False}, ("eax.long", 3, 1, 16384)),
    ("eax_siv_plan", (False, 64 * MIB), {"decrypt": True}, ("eax.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 64 * MIB), {"decrypt": False}, ("s2v.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, 64 * MIB), {"decrypt": True}, ("s2v.long", 2, 1, 16384)),
    ("chain_plan", ("cbc", 64 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", 64 * MIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("chain_plan", ("cfb", 64 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", 64 * MIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("chain_plan", ("ofb", 64 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", 64 * MIB), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 64 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", 64 * MIB), {"decrypt": True}, None),
    ("chain_plan", ("ccm", 64 * MIB), {"decrypt": False}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("ccm", 64 * MIB), {"decrypt": True}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("cbc_nocts", 64 * MIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", 64 * MIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("plan", ("ecb", GIB), {}, ("ecb.tiled", 1, 256, 0)),
    ("plan", ("ecb", GIB), {"direction": 1}, ("ecb.tiled", 1, 256, 0)),
    ("plan", ("ctr", GIB), {}, ("ctr.striped", 1, 256, 0)),
    ("plan", ("xts", GIB, 1), {}, ("xts.bulk", 3, 0, 0)),
    ("plan", ("gcm", GIB), {}, ("gcm.striped", 3, 256, 0)),
    ("plan", ("gcm", GIB), {"direction": 1}, ("gcm.levels", 5, 0, 0)),
    ("plan", ("gcm", GIB, 37), {}, ("gcm.striped", 3, 256, 0)),
    ("plan", ("gcm", GIB), {"counter": J0}, ("gcm.striped", 3, 256, 0)),
    ("plan", ("ctr", GIB), {"counter": J0}, ("ctr.striped", 1, 256, 0)),
    ("plan", ("siv", GIB), {}, ("siv.levels", 7, 0, 0)),
    ("plan", ("siv", GIB), {"direction": 1}, ("siv.levels", 7, 0, 0)),
    ("plan", ("ocb", GIB), {}, ("ocb.runs", 1, 0, 0)),
    ("plan", ("ocb", GIB), {"direction": 1}, ("ocb.runs", 1, 0, 0)),
    ("poly1305_plan", (GIB,), {}, ("poly.chunks", 2, 2048, 128)),
    ("plan", ("xts", 4096, 262144), {}, ("xts.bulk", 2, 0, 0)),
    ("plan", ("xts", 512, 2097152), {}, ("xts.packed", 2, 0, 0)),
    ("eax_siv_plan", (False, GIB), {"decrypt": False}, ("eax.long", 3, 1, 16384)),
    ("eax_siv_plan", (False, GIB), {"decrypt": True}, ("eax.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, GIB), {"decrypt": False}, ("s2v.long", 2, 1, 16384)),
    ("eax_siv_plan", (True, GIB), {"decrypt": True}, ("s2v.long", 2, 1, 16384)),
    ("chain_plan", ("cbc", GIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc", GIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("chain_plan", ("cfb", GIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cfb", GIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("chain_plan", ("ofb", GIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("ofb", GIB), {"decrypt": True}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", GIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cmac", GIB), {"decrypt": True}, None),
    ("chain_plan", ("ccm", GIB), {"decrypt": False}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("ccm", GIB), {"decrypt": True}, ("ccm.split", 2, 1, 64)),
    ("chain_plan", ("cbc_nocts", GIB), {"decrypt": False}, ("chain.serial", 1, 1, 64)),
    ("chain_plan", ("cbc_nocts", GIB), {"decrypt": True}, ("fbdec.tiled", 1, 256, 1024)),
    ("poly1305_plan", (64, 1), {}, ("poly.small", 1, 1, 1)),
    ("chain_plan", ("cbc_batch", 64, 1), {}, ("batch.row", 1, 1, 256)),
    ("chain_plan", ("cmac_batch", 64, 1), {}, ("batch.row", 1, 1, 256)),
    ("eax_siv_plan", (False, 64, 1), {"decrypt": False}, ("eax.small", 1, 1, 16384)),
    ("eax_siv_plan", (False, 64, 1), {"decrypt": True}, ("eax.small", 1, 1, 16384)),
    ("eax_siv_plan", (True, 64, 1), {"decrypt": False}, ("s2v.small", 1, 1, 16384)),
    ("eax_siv_plan", (True, 64, 1), {"decrypt": True}, ("s2v.small", 1, 1, 16384)),
    ("poly1305_plan", (64, 8192), {}, ("poly.batch", 1, 2048, 1)),
    ("chain_plan", ("cbc_batch", 64, 8192), {}, ("batch.row", 1, 256, 256)),
    ("chain_plan", ("cmac_batch", 64, 8192), {}, ("batch.row", 1, 256, 256)),
    ("eax_siv_plan", (False, 64, 8192), {"decrypt": False}, ("eax.batch", 1, 256, 16384)),
    ("eax_siv_plan", (False, 64, 8192), {"decrypt": True}, ("eax.batch", 1, 256, 16384)),
    ("eax_siv_plan", (True, 64, 8192), {"decrypt": False}, ("s2v.batch", 1, 256, 16384)),
    ("eax_siv_plan", (True, 64, 8192), {"decrypt": True}, ("s2v.batch", 1, 256, 16384)),
    ("poly1305_plan", (64, 8193), {}, ("poly.batch", 1, 2048, 1)),
    ("chain_plan", ("cbc_batch", 64, 8193), {}, ("batch.row", 1, 129, 1024)),
    ("chain_plan", ("cmac_batch", 64, 8193), {}, ("batch.row", 1, 129, 1024)),
    ("eax_siv_plan", (False, 64, 8193), {"decrypt": False}, ("eax.batch", 1, 129, 16384)),
    ("eax_siv_plan", (False, 64, 8193), {"decrypt": True}, ("eax.batch", 1, 129, 16384)),
    ("eax_siv_plan", (True, 64, 8193), {"decrypt": False}, ("s2v.batch", 1, 129, 16384)),
    ("eax_siv_plan", (True, 64, 8193), {"decrypt": True}, ("s2v.batch", 1, 129, 16384)),
    ("poly1305_plan", (64, 81920), {}, ("poly.batch", 1, 2048, 1)),
    ("chain_plan", ("cbc_batch", 64, 81920), {}, ("batch.lane", 1, 80, 1024)),
    ("chain_plan", ("cmac_batch", 64, 81920), {}, ("batch.lane", 1, 80, 1024)),
    ("eax_siv_plan", (False, 64, 81920), {"decrypt": False}, ("eax.batch", 1, 256, 16384)),
    ("eax_siv_plan", (False, 64, 81920), {"decrypt": True}, ("eax.batch", 1, 256, 16384)),
    ("eax_siv_plan", (True, 64, 81920), {"decrypt": False}, ("s2v.batch", 1, 256, 16384)),
    ("eax_siv_plan", (True, 64, 81920), {"decrypt": True}, ("s2v.batch", 1, 256, 16384)),
]


def _answer(hook, args, kw):
    try:
        return getattr(uaes, hook)(*args, **kw)
    except ValueError:
        return None


def test_the_table_covers_every_hook_size_and_count():
    sizes = {16, 4096, MIB, 8 * MIB - 16, 8 * MIB, 20 * MIB, 64 * MIB, GIB}
    for mode in ("ecb", "ctr", "xts", "gcm", "siv", "ocb"):
        assert {a[1] for h, a, kw, _ in EXPECTED if h == "plan" and a[0] == mode and (mode != "xts" or a[2] == 1)} == sizes, mode
    assert {kw.get("direction", 0) for h, a, kw, _ in EXPECTED if h == "plan" and a[0] == "gcm"} == {0, 1}
    assert any(h == "plan" and a[0] == "gcm" and kw.get("counter", b"\0")[-1] for h, a, kw, _ in EXPECTED)
    assert {a[0] for h, a, kw, _ in EXPECTED if h == "poly1305_plan" and len(a) == 1} == sizes
    assert {a[1] for h, a, kw, _ in EXPECTED if h == "eax_siv_plan" and len(a) == 2} == sizes
    assert {a[1] for h, a, kw, _ in EXPECTED if h == "chain_plan" and len(a) == 2} == sizes
    for hook in ("poly1305_plan", "eax_siv_plan", "chain_plan"):
        assert {a[-1] for h, a, kw, _ in EXPECTED if h == hook and len(a) == (2 if hook == "poly1305_plan" else 3)} == {1, 8192, 8193, 81920}, hook


@pytest.mark.parametrize("hook", ["plan", "poly1305_plan", "eax_siv_plan", "chain_plan"])
def test_planning_is_what_it_was(hook):
    got = [(args, kw, want, _answer(hook, args, kw)) for h, args, kw, want in EXPECTED if h == hook]
    assert got
    wrong = [g for g in got if g[3] != g[2]]
    assert not wrong, wrong[:8]


# uaes.plan_gcm_piece(len, done, decrypt): what uaes_gcm_stream_update runs for one piece of a streamed GCM message, from
# the function uaesk_gcm_stream_piece switches on (gcm_piece_plan, csrc/uaes_gcm.hip).  Worked by hand from gcm_plan for 256
# CUs: no chunk workgroups below 1024 GHASH positions ("gcm.levels", 0 launches: the absorb path), then one launch of
# ceil(positions / (1024 * steps)) chunk workgroups with the smallest power-of-two steps that fits 256 of them, two
# phases past 2^20 positions, the striped pass past 2^23 (three launches, five for a decryption: the tail's CTR kernel and
# its GHASH come apart).  A ragged piece counts its last block.
KIB = 1024
PIECE_EXPECTED = [
    ((16,), ("gcm.levels", 0, 0, 0)),
    ((16 * KIB - 16,), ("gcm.levels", 0, 0, 0)),
    ((16 * KIB - 3,), ("gcm.chunks", 1, 1, 1)),
    ((16 * KIB,), ("gcm.chunks", 1, 1, 1)),
    ((16 * KIB + 1,), ("gcm.chunks", 1, 2, 1)),
    ((16 * KIB, 16 * 253, True), ("gcm.chunks", 1, 1, 1)),
    ((4 * MIB,), ("gcm.chunks", 1, 256, 1)),
    ((4 * MIB + 16,), ("gcm.chunks", 1, 129, 2)),
    ((8 * MIB,), ("gcm.chunks", 1, 256, 2)),
    ((8 * MIB + 16,), ("gcm.chunks", 1, 129, 4)),
    ((16 * MIB,), ("gcm.chunks", 1, 256, 4)),
    ((16 * MIB, 0, True), ("gcm.chunks", 1, 256, 4)),
    ((16 * MIB + 16,), ("gcm.twophase", 2, 129, 8)),
    ((16 * MIB + 16, 16 * 254, True), ("gcm.twophase", 2, 129, 8)),
    ((64 * MIB,), ("gcm.twophase", 2, 256, 16)),
    ((128 * MIB,), ("gcm.twophase", 2, 256, 32)),
    ((128 * MIB + 16,), ("gcm.striped", 3, 256, 0)),
    ((128 * MIB + 16, 0, True), ("gcm.striped", 5, 256, 0)),
    ((128 * MIB + 16, 16 * 254), ("gcm.striped", 3, 256, 0)),
    ((128 * MIB + 16, 128 * MIB + 32 * KIB + 16, True), ("gcm.striped", 5, 256, 0)),
    ((GIB,), ("gcm.striped", 3, 256, 0)),
]


def test_piece_planning_without_a_device():
    got = [(args, want, uaes.plan_gcm_piece(*args)) for args, want in PIECE_EXPECTED]
    wrong = [g for g in got if g[2] != g[1]]
    assert not wrong, wrong
    # up to the two phases a piece is planned like a one-shot encryption of the same length without its small arrangement
    for n in (MIB, 4 * MIB + 16, 16 * MIB, 16 * MIB + 16, 128 * MIB):
        piece, whole = uaes.plan_gcm_piece(n), uaes.plan("gcm", n)
        assert (piece[0], piece[2], piece[3]) == (whole[0], whole[2], whole[3]), n
    with pytest.raises(uaes.EngineError):
        uaes.plan_gcm_piece(4096, done=8)
    # with the chunk arrangements switched off a piece is striped from one stripe per CU on, counted from its first group
    L = uaes.engine()
    off = (1 << uaes.arrangement_id("gcm.chunks")) | (1 << uaes.arrangement_id("gcm.twophase"))
    try:
        L.uaes_debug_plan_disable(off)
        for done, h0 in ((0, 254), (16 * 253, 1), (16 * 254, 0), (16 * 255, 255)):
            n = 16 * (h0 + 2048 * 256)
            assert uaes.plan_gcm_piece(n, done) == ("gcm.striped", 3, 256, 0), (done, h0)
            assert uaes.plan_gcm_piece(n - 16, done) == ("gcm.levels", 0, 0, 0), (done, h0)
    finally:
        L.uaes_debug_plan_disable(0)
