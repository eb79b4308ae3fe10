#!/usr/bin/env python3
"""What an animation step costs under the dual-quaternion rule (include/pt_skin_dq.h: the posed binding 3, the refit, the patch and the motion
records all on the device) against pt_move_geometry fed pt_pose_triangles' output of the same DQ pose, which is the parent's unchanged code
path.  The timing is scripts/skin_bench.py's, with the skin route's pose made by pt_skin_dq_create.

usage: skin_dq_bench.py                 one child process per part (timing m6, scripts/skin_dq_probe.py c4, timing big, skin_dq_probe.py big);
                                        everything printed is also written to profiles/r35_skin_dq.txt
       skin_dq_bench.py timing m6|big   M6 (scenes.m6_twisting) with its tube tessellated to about 100 k triangles, 8 joints | the
                                        1 002 528-triangle height field of scripts/big_scene.py in the 7 bands of scripts/pose_bench.py, each
                                        corner ramped between its band's joint and the next one's"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "r35_skin_dq.txt")

if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        import skin_bench as SB
        SB.timing(sys.argv[2], blend="dq")
    else:
        lines = []
        here = os.path.dirname(os.path.abspath(__file__))
        for script, part in (("skin_dq_bench.py", ("timing", "m6")), ("skin_dq_probe.py", ("c4",)), ("skin_dq_bench.py", ("timing", "big")), ("skin_dq_probe.py", ("big",))):
            print(f"[{script} {' '.join(part)} ...]", flush=True)
            p = subprocess.run([sys.executable, os.path.join(here, script)] + list(part), capture_output=True, text=True, timeout=900)
            for line in p.stdout.splitlines():
                print(line, flush=True)
                lines.append(line)
            if p.returncode != 0:
                print(p.stderr[-2000:], flush=True)
                sys.exit(f"{script} {' '.join(part)} ended with {p.returncode}: nothing further is started")
            if part[-1] == "c4":
                lines.append("")
        with open(OUT, "w") as f:
            f.write("scripts/skin_dq_bench.py: an animation step under the dual-quaternion rule (pt_skin_dq_create + pt_pose_geometry; the lines say 'skin route') against pt_move_geometry fed the same triangles\n")
            f.write("scripts/skin_dq_probe.py: k_dq_records + k_skin_dq_corners beside k_skin_corners on the device (pt_debug_skin_dq_time, pt_debug_skin_time)\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
