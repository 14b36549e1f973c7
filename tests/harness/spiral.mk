# tests/harness/spiral.mk — ASan + UBSan build of spiral_check (tests/test_spiral_core.py): JM's
# spiral order as csrc/jmh_spiral.h states it, against the loops of Init_Motion_Search_Module and
# the table fill it replaced.   make -C tests/harness -f spiral.mk
CC       ?= gcc
ASAN     := _build_asan
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O2 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all

$(ASAN)/spiral_check: spiral_check.c $(CSRC)/jmh_spiral.h
	mkdir -p $(ASAN)
	$(CC) -std=gnu11 -Wall -Wno-unused-function $(SANFLAGS) spiral_check.c -o $@
