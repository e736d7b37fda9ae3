"""A FIFO as the output file of a writer under test, read by the test itself without a second thread.  Test infrastructure only.

The test holds the read end open (O_NONBLOCK, so that opening does not wait for a writer) from before the call until it has read
everything; the writer's bytes wait in the pipe.  A writer blocks only on a full pipe, so the bytes expected must fit the pipe's
capacity, which is checked BEFORE the call: a test that would have hung fails instead."""
import contextlib
import fcntl
import os


@contextlib.contextmanager
def fifo_reader(path, expect_bytes):
    "makes the FIFO `path`; yields drain() -> everything written to it so far, up to the end of file (call it when the writer has closed)"
    os.mkfifo(path)
    fd = os.open(path, os.O_RDONLY | os.O_NONBLOCK)
    try:
        room = fcntl.fcntl(fd, fcntl.F_GETPIPE_SZ)
        assert expect_bytes < room, f"{expect_bytes} bytes would not fit the pipe's {room}: the writer would wait for a reader"

        def drain():
            got = b""
            while True:
                part = os.read(fd, 1 << 16)  # (no writer left and nothing buffered: b"", the end of file)
                if not part:
                    return got
                got += part
        yield drain
    finally:
        os.close(fd)
    assert os.path.exists(path)  # (never removed, complete or not)
